"""The demo module's gate normalisation inside the K x K engine (cspn2d_*_kxk_absnorm_*, cspn_amd/csrc/cspn2d_kxk.hip):
the raw guide goes where the gates went, |g| enters the multiply-add, the sum is scaled by 1 / S after it, and no normalised gate or
dL/dw tensor exists.
  CPU  the five symbols, the ABI version, __all__, the argument errors of the unfused twins, the byte counts
  1.   forward, every kept level and both gradients against the float64 statement of the module (test_kernel_size._torch_module) on
       the non-square tile grids of test_kxk_tilegrid
  2.   fp16 / bf16 guides: out and dL/dx bitwise the float32 call's on guide.float(), dL/dguide bitwise its float32 value rounded once
  3.   all-zero slices: the NaN pattern of the float64 statement
  4.   <F x, y> == <x, F^T y>
  5.   CSPN and absnorm_propagate are the functional calls on the folded views
  6.   no temporary of the gates' size
  7.   a captured graph replays the eager result
Tolerances: 1e-5 of max|ref| forward (test_kernel_size.test_cspn_module_vs_fp64_torch), helpers.assert_close(rtol=2e-4, atol_frac=5e-6)
for gradients, 2e-4 of sum |F x y| for the adjoint identity.  Each comparison prints its error as a fraction of its bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F
from helpers import assert_close
from test_kernel_size import _misaligned, _torch_module
from test_kxk_tilegrid import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_forward_kxk_absnorm_f32", "cspn2d_forward_kxk_absnorm_g16", "cspn2d_backward_kxk_absnorm_f32",
       "cspn2d_backward_kxk_absnorm_g16", "cspn2d_backward_kxk_absnorm_workspace_bytes"]
RTOL = 1e-5
GTOL, GFLOOR = 2e-4, 5e-6
ATOL_ADJ = 2e-4
DTYPES16 = [torch.float16, torch.bfloat16]
N = 2


def _guide(n, K, H, W, seed, dtype=torch.float32):
    """(rand + 0.05) sign: any sign, and no abs-sum is tiny"""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.rand(n, K * K - 1, H, W, generator=gen) + 0.05
    sign = (torch.rand(n, K * K - 1, H, W, generator=gen) < 0.5).float() * 2 - 1
    return (mag * sign).to(dtype)


def _values(n, C, H, W, seed):
    return torch.rand(n, C, H, W, generator=torch.Generator().manual_seed(seed)) * 4 - 1


def _statement(gt, xt, K, n):
    """the float64 module on a guide that the C channels share: channel c's slice is the guide itself"""
    return _torch_module(gt.repeat(1, xt.shape[1], 1, 1), xt, K, n)


def _fwd(a, ref, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    e = float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))
    print("absnorm fwd  %-44s %.3g of %g" % (what, e / RTOL, RTOL))
    assert np.isfinite(a).all() and e <= RTOL, "%s: relative error %.3g > %g" % (what, e, RTOL)


def _grad(a, ref, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    bound = GFLOOR * max(np.abs(ref[fin]).max(), 1e-30) + GTOL * np.abs(ref[fin])
    print("absnorm grad %-44s %.3g of the bound" % (what, float((np.abs(a[fin] - ref[fin]) / bound).max())))
    assert_close(a, ref, what, rtol=GTOL, atol_frac=GFLOOR)


def _bits(a, b):
    """the same dtype, shape and bit pattern (NaN payloads included)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


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
    assert {"cspn2d_forward_kxk_absnorm", "cspn2d_backward_kxk_absnorm"} <= set(cspn_amd.__all__)
    assert cspn_amd.cspn2d_forward_kxk_absnorm is F.cspn2d_forward_kxk_absnorm
    assert cspn_amd.cspn2d_backward_kxk_absnorm is F.cspn2d_backward_kxk_absnorm


def test_backward_workspace_bytes():
    ours = _lib.late_symbol("cspn2d_backward_kxk_absnorm_workspace_bytes")
    twin = _lib.late_symbol("cspn2d_backward_kxk_workspace_bytes")
    B, C, H, W = 2, 3, 10, 13
    for K in (5, 7):
        for n in (2, 3, 24):
            # the twin's adjoint levels and one float32 plane of 1 / S, at most 256 bytes of padding
            assert twin(B, C, H, W, K, n) + 4 * B * H * W <= ours(B, C, H, W, K, n) <= twin(B, C, H, W, K, n) + 4 * B * H * W + 256
            assert ours(B, C, H, W, K, n) % 256 == 0
        for n in (0, 1, -1):
            assert twin(B, C, H, W, K, n) == 0 and ours(B, C, H, W, K, n) == 0
    for K in (3, 4, 9, 0):
        assert twin(B, C, H, W, K, 4) == 0 and ours(B, C, H, W, K, 4) == 0
    for shape in ((0, 3, 10, 13), (2, 0, 10, 13), (2, 3, 0, 13), (2, 3, 10, 0)):
        assert twin(*shape, 5, 4) == 0 and ours(*shape, 5, 4) == 0
    assert twin(1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3) == 0 and ours(1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3) == 0


def test_argument_errors_are_those_of_the_unfused_twins():
    """no call below reaches a launch: every one fails a check (or, need nothing, returns 0) before the stream is touched"""
    g, x, o, h, w, gg, gx = (ctypes.c_void_p(i << 32) for i in range(1, 8))
    odd = ctypes.c_void_p((1 << 32) + 1)
    hbytes = 4 * 2 * 8 * 8 * 2
    big = 1 << 20
    # (gate, x, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
    fwd = [((g, x, o, None, 0, 2, 1, 8, 8, K, 3, w, big, None), -1) for K in (3, 4, 9, 0)] + [
        ((None, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, None, o, None, 0, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, x, None, None, 0, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, x, o, None, 0, 0, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, x, o, None, 0, 1, 0, 8, 8, 5, 3, w, big, None), -1),
        ((g, x, o, None, 0, 1, 1, 8, 0, 5, 3, w, big, None), -1),
        ((g, x, o, None, 0, 2, 1, 8, 8, 5, -1, w, big, None), -1),
        ((g, x, x, None, 0, 2, 1, 8, 8, 7, 3, w, big, None), -1),
        ((g, x, g, None, 0, 2, 1, 8, 8, 7, 3, w, big, None), -1),
        ((g, x, o, x, big, 2, 1, 8, 8, 5, 3, None, 0, None), -1),
        ((g, x, o, None, 0, 2, 1, 8, 8, 5, 3, None, 0, None), -2),
        ((g, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, 100, None), -2),
        ((g, x, o, None, 0, 2, 1, 8, 8, 5, 3, ctypes.c_void_p((6 << 32) + 4), big, None), -2),
        ((g, x, o, h, 100, 2, 1, 8, 8, 5, 3, None, 0, None), -2),
        ((g, x, o, None, 0, 1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3, w, big, None), -3),
        ((g, x, o, None, 0, 1 << 8, 1, 1 << 10, 1 << 8, 7, 3, w, big, None), -3)]
    # (gate, x, history, history_bytes, grad_out, grad_gate, grad_x, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
    bwd = [((g, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 9, 3, w, big, None), -1),
           ((None, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, hbytes, None, gg, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, hbytes, o, gg, gx, 2, 1, 0, 8, 5, 3, w, big, None), -1),
           ((g, x, None, 0, o, gg, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, 64, o, gg, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, hbytes, o, gg, gg, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, hbytes, o, gg, o, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, hbytes, o, x, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, hbytes, o, gg, h, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, None, 0, None), -2),
           ((g, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, 64, None), -2),
           ((g, x, h, hbytes, o, gg, gx, 1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3, w, big, None), -3),
           ((g, x, h, hbytes, o, None, None, 2, 1, 8, 8, 5, 3, w, big, None), 0)]   # nothing asked for: nothing done
    for kind, cases in (("forward", fwd), ("backward", bwd)):
        twin32, ours32 = (_lib.late_symbol("cspn2d_%s_kxk%s_f32" % (kind, s)) for s in ("", "_absnorm"))
        twin16, ours16 = (_lib.late_symbol("cspn2d_%s_kxk%s_g16" % (kind, s)) for s in ("", "_absnorm"))
        for args, code in cases:
            assert twin32(*args) == code == ours32(*args), (kind, args)
            for dt in (1, 2):
                a16 = (args[0], dt) + args[1:]
                assert twin16(*a16) == code == ours16(*a16), (kind, dt, args)
        ok = cases[0][0][:9 if kind == "forward" else 11] + (5,) + cases[0][0][10 if kind == "forward" else 12:]
        for dt in (0, 3, -1):   # a dtype that is neither fp16 nor bf16
            a16 = (ok[0], dt) + ok[1:]
            assert twin16(*a16) == -1 == ours16(*a16)
            assert b"dtype" in cspn_amd.load().cspn_last_error()
        a16 = (odd, 1) + ok[1:]   # a 16-bit tensor at an odd address
        assert twin16(*a16) == -1 == ours16(*a16)


def test_python_argument_errors_without_gpu():
    g, x = torch.zeros(1, 24, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk_absnorm(g, x, 3, 2)          # the 3 x 3 op is not this engine
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk_absnorm(g, x, 7, 2)          # 24 channels are not 7 x 7
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk_absnorm(g, x, 5, -1)
    with pytest.raises(ValueError):
        F.cspn2d_backward_kxk_absnorm(g, x, x[:, :1], 5, 2)
    with pytest.raises(_lib.CspnError):
        F.cspn2d_forward_kxk_absnorm(g, x, 5, 2)          # no CPU path
    assert F.cspn2d_forward_kxk_absnorm(g, x, 5, 0) is x


# ---- 1. against the float64 statement ----
_REF = {}


def _reference(name, K, C, n=6):
    """(guide, x, grad_out, levels H_1 .. H_n, dL/dguide, dL/dx) of the float64 statement, computed once per case"""
    key = (name, K, C, n)
    if key not in _REF:
        H, W = SHAPES[name]
        g, x, go = _guide(N, K, H, W, K * 1000 + W + C), _values(N, C, H, W, H + K), _values(N, C, H, W, 7 + W)
        gt, xt = g.double().requires_grad_(True), x.double().requires_grad_(True)
        out = _statement(gt, xt, K, n)
        out.backward(go.double())
        with torch.no_grad():
            lv = [_statement(gt, xt, K, t) for t in range(1, n)] + [out.detach()]
        _REF[key] = (g, x, go, lv, gt.grad, xt.grad)
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("name", ["wide", "tall", "strip"])
def test_forward_levels_and_gradients_vs_fp64(name, K, C):
    (H, W), n = SHAPES[name], 6
    g, x, go, lv, rg, rx = _reference(name, K, C)
    what = "%s K=%d C=%d" % (name, K, C)
    gd, xd, god = g.cuda(), x.cuda(), go.cuda()
    out = F.cspn2d_forward_kxk_absnorm(gd, xd, K, n)
    _fwd(out.cpu(), lv[-1], what)
    out_h, hist = F.cspn2d_forward_kxk_absnorm(gd, xd, K, n, return_history=True)
    assert torch.equal(out_h, out), "the forward that keeps its levels gives other bits"
    kept = hist.view(n - 1, N, C, H, W)
    for t in range(n - 1):
        _fwd(kept[t].cpu(), lv[t], what + " level %d" % (t + 1))
    gg, gx = F.cspn2d_backward_kxk_absnorm(gd, xd, god, K, n)
    assert gg.shape == gd.shape and gx.shape == xd.shape
    _grad(gg.cpu(), rg, what + " dL/dguide")   # summed over the C channels
    _grad(gx.cpu(), rx, what + " dL/dx")
    gg_h, gx_h = F.cspn2d_backward_kxk_absnorm(gd, xd, god, K, n, hist)
    assert torch.equal(gg_h, gg) and torch.equal(gx_h, gx), "the kept history gives other gradients than the recomputed one"
    gg2, gx2 = F.cspn2d_backward_kxk_absnorm(gd, xd, god, K, n)
    assert torch.equal(gg2, gg) and torch.equal(gx2, gx), "the backward is not deterministic"


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_float32_views_one_element_off_alignment_give_the_same_bits(K):
    """W % 4 == 0, every tensor 4 bytes past a 16-byte boundary: the guarded scalar instances against the vector ones"""
    (H, W), C, n = SHAPES["wide"], 2, 3
    g, x, go = _reference("wide", K, C)[:3]
    gd, xd, god = g.cuda(), x.cuda(), go.cuda()
    out, (gg, gx) = F.cspn2d_forward_kxk_absnorm(gd, xd, K, n), F.cspn2d_backward_kxk_absnorm(gd, xd, god, K, n)
    gm, xm, gom = _misaligned(g), _misaligned(x), _misaligned(go)
    assert torch.equal(F.cspn2d_forward_kxk_absnorm(gm, xm, K, n), out)
    ggm, gxm = F.cspn2d_backward_kxk_absnorm(gm, xm, gom, K, n)
    assert torch.equal(ggm, gg) and torch.equal(gxm, gx)


# ---- 2. fp16 / bf16 guides ----
def _off_by_one(t):
    """a device copy of t that starts one element (2 bytes) past an allocation's base"""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 != 0
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("layout", ["wide", "strip", "wide+1"])
@pytest.mark.parametrize("dtype", DTYPES16)
def test_16_bit_guides_are_bitwise_the_float32_call_on_the_widened_guide(dtype, layout, K):
    name = layout.split("+")[0]
    (H, W), C, n = SHAPES[name], 2, 3
    g16 = _guide(N, K, H, W, K * 77 + W, dtype).cuda()
    if layout.endswith("+1"):
        g16 = _off_by_one(g16)
    g32 = g16.float()
    x, go = _values(N, C, H, W, 3 + K).cuda(), _values(N, C, H, W, 5 + K).cuda()
    for steps in (n, 1):
        out16, h16 = F.cspn2d_forward_kxk_absnorm(g16, x, K, steps, return_history=True)
        out32, h32 = F.cspn2d_forward_kxk_absnorm(g32, x, K, steps, return_history=True)
        assert out16.dtype == torch.float32 and torch.equal(out16, out32) and bool(out16.isfinite().all())
        assert torch.equal(F.cspn2d_forward_kxk_absnorm(g16, x, K, steps), out32)
        if steps > 1:
            assert torch.equal(h16, h32)
        gg16, gx16 = F.cspn2d_backward_kxk_absnorm(g16, x, go, K, steps, h16)
        gg32, gx32 = F.cspn2d_backward_kxk_absnorm(g32, x, go, K, steps, h32)
        assert gx16.dtype == torch.float32 and torch.equal(gx16, gx32)
        assert gg16.dtype == dtype and _bits(gg16, gg32.to(dtype)) and bool((gg16 != 0).any()) and bool(gg16.isfinite().all())
        only_g, none = F.cspn2d_backward_kxk_absnorm(g16, x, go, K, steps, h16, need_x=False)
        assert none is None and _bits(only_g, gg16)
        none, only_x = F.cspn2d_backward_kxk_absnorm(g16, x, go, K, steps, need_guide=False)
        assert none is None and torch.equal(only_x, gx32)


# ---- 3. all-zero slices ----
@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_all_zero_slices_give_the_nan_pattern_of_the_fp64_statement(K):
    """image 0: a pixel inside a tile; image 1: the pixel at the corner of an interior tile seam (rows 15 | 16, columns 63 | 64)"""
    (H, W), C, n = SHAPES["wide"], 2, 2
    g = _guide(N, K, H, W, K + 90)
    g[0, :, 7, 30] = 0
    g[1, :, 16, 64] = 0
    x, go = _values(N, C, H, W, 91), _values(N, C, H, W, 92)
    gt, xt = g.double().requires_grad_(True), x.double().requires_grad_(True)
    ref = _statement(gt, xt, K, n)
    ref.backward(go.double())
    assert bool(ref.isnan().any()) and not bool(ref.isnan().all())
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        # (the 16-bit guides: the same zeros, other roundings of the rest; compared against their own widened statement)
        gd = g.to(dtype).cuda()
        if dtype == torch.float32:
            r_out, r_g, r_x = ref.detach(), gt.grad, xt.grad
        else:
            g2 = gd.cpu().double().requires_grad_(True)
            x2 = x.double().requires_grad_(True)
            r_out = _statement(g2, x2, K, n)
            r_out.backward(go.double())
            r_out, r_g, r_x = r_out.detach(), g2.grad, x2.grad
        what = "zero slices K=%d %s" % (K, dtype)
        out = F.cspn2d_forward_kxk_absnorm(gd, x.cuda(), K, n).cpu()
        gg, gx = F.cspn2d_backward_kxk_absnorm(gd, x.cuda(), go.cuda(), K, n)
        gg, gx = gg.float().cpu(), gx.cpu()
        for a, r, nm in ((out, r_out, "out"), (gg, r_g, "dL/dguide"), (gx, r_x, "dL/dx")):
            assert torch.equal(a.isnan(), r.isnan()), "%s %s: %d NaNs, the statement has %d" % (what, nm, int(a.isnan().sum()), int(r.isnan().sum()))
            assert bool((a.isfinite() | a.isnan()).all()) and bool(r.isnan().any())
        fin = ~r_out.isnan()
        _fwd(out[fin], r_out[fin], what)
        _grad(gx.numpy(), r_x.numpy(), what + " dL/dx")
        if dtype == torch.float32:   # (a 16-bit gradient carries its own rounding: checked bitwise in test 2)
            _grad(gg.numpy(), r_g.numpy(), what + " dL/dguide")


# ---- 4. adjointness ----
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("name", ["tall", "strip"])
def test_step_and_adjoint_step_are_adjoint(name, K, n):
    (H, W), C = SHAPES[name], 2
    g = _guide(N, K, H, W, K * 7 + n).cuda()
    x, y = _values(N, C, H, W, W + n).cuda(), _values(N, C, H, W, H + n).cuda()
    fx = F.cspn2d_forward_kxk_absnorm(g, x, K, n)
    none, bty = F.cspn2d_backward_kxk_absnorm(g, x, y, K, n, need_guide=False)
    assert none is None
    lhs, rhs = float((fx.double() * y.double()).sum()), float((x.double() * bty.double()).sum())
    scale = float((fx.double() * y.double()).abs().sum())
    print("absnorm adj  %-44s %.3g of the bound" % ("%s K=%d n=%d" % (name, K, n), abs(lhs - rhs) / (ATOL_ADJ * scale)))
    assert np.isfinite(lhs) and np.isfinite(rhs) and scale > 0
    assert abs(lhs - rhs) <= ATOL_ADJ * scale, "<F x, y> = %.9g, <x, F^T y> = %.9g, sum |F x y| = %.6g" % (lhs, rhs, scale)


# ---- 5. the routes ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32] + DTYPES16)
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("ks", [5, 7])
def test_module_and_absnorm_propagate_are_the_functional_calls_on_the_folded_views(ks, C, dtype):
    (H, W), n, KK = (20, 68), 3, ks * ks - 1
    guide = torch.cat([_guide(N, ks, H, W, ks + 10 * c) for c in range(C)], 1).to(dtype).cuda()   # every channel its own slice
    feat, go = _values(N, C, H, W, 11).cuda(), _values(N, C, H, W, 12).cuda()
    gf, xf, gof = guide.view(N * C, KK, H, W), feat.view(N * C, 1, H, W), go.view(N * C, 1, H, W)
    out, hist = F.cspn2d_forward_kxk_absnorm(gf, xf, ks, n, return_history=True)
    gg, gx = F.cspn2d_backward_kxk_absnorm(gf, xf, gof, ks, n, hist)
    for route in (cspn_amd.CSPN(2, C, ks, n), lambda a, b: cspn_amd.absnorm_propagate(a, b, n, ks)):
        with torch.no_grad():
            assert torch.equal(route(guide, feat), out.view(N, C, H, W))
        gr, fr = guide.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        y = route(gr, fr)
        assert y.dtype == torch.float32 and torch.equal(y.detach(), out.view(N, C, H, W))
        y.backward(go)
        assert gr.grad.dtype == dtype and _bits(gr.grad, gg.view(N, C * KK, H, W))
        assert torch.equal(fr.grad, gx.view(N, C, H, W))
        # one gradient alone
        gr = guide.clone().requires_grad_(True)
        route(gr, feat).backward(go)
        assert _bits(gr.grad, gg.view(N, C * KK, H, W))
    if dtype != torch.float32:   # a 16-bit feat is widened with one cast
        assert torch.equal(cspn_amd.CSPN(2, C, ks, n)(guide, feat.to(dtype)), cspn_amd.CSPN(2, C, ks, n)(guide, feat.to(dtype).float()))


# ---- 6. no temporary of the gates' size ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_the_module_allocates_no_tensor_of_the_gates_size(dtype):
    """peak memory over the call, less what was there before and what the call returns, stays below one float32 copy of the gates
    (4 KK N C H W bytes).  With n = 4 the kept levels (3), the adjoint levels (3), the plane of 1 / S and the contiguous grad_out are
    8 planes of 4 bytes per pixel against KK = 24."""
    ks, n, C, H, W = 5, 4, 2, 64, 256
    KK = ks * ks - 1
    assert N * C * H * W >= 64 * 1024
    bound = 4 * KK * N * C * H * W
    m = cspn_amd.CSPN(2, C, ks, n)
    guide = _guide(N, ks, H, W, 5).repeat(1, C, 1, 1).to(dtype).cuda()
    feat, go = _values(N, C, H, W, 6).cuda(), _values(N, C, H, W, 7).cuda()

    def nbytes(*ts):
        return sum(t.numel() * t.element_size() for t in ts)

    gr, fr = guide.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    m(gr, fr).backward(go)   # warm: symbols bound, the allocator's pools filled
    gr.grad = fr.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = m(guide, feat)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - nbytes(out)
    print("absnorm mem  forward %s: %d bytes beyond the output, %.3g of the bound %d" % (dtype, extra, extra / bound, bound))
    assert extra < bound
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = m(gr, fr)
    out.backward(go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - nbytes(out, gr.grad, fr.grad)
    print("absnorm mem  forward + backward %s: %d bytes beyond the output and the gradients, %.3g of the bound %d" % (dtype, extra, extra / bound, bound))
    assert gr.grad.dtype == dtype and extra < bound


# ---- 7. a captured graph ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_captured_graph_replays_the_eager_result(dtype):
    K, C, (H, W), n = 5, 2, (40, 136), 4
    g, g2 = _guide(N, K, H, W, 40, dtype).cuda(), _guide(N, K, H, W, 41, dtype).cuda()
    x, go = _values(N, C, H, W, 42).cuda(), _values(N, C, H, W, 43).cuda()
    r_out, r_hist = F.cspn2d_forward_kxk_absnorm(g, x, K, n, return_history=True)
    r_gg, r_gx = F.cspn2d_backward_kxk_absnorm(g, x, go, K, n, r_hist)
    r2 = F.cspn2d_forward_kxk_absnorm(g2, x, K, n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # one stream, one chain: forward, then backward on its history
        c_out, c_hist = F.cspn2d_forward_kxk_absnorm(g, x, K, n, return_history=True)
        c_gg, c_gx = F.cspn2d_backward_kxk_absnorm(g, x, go, K, n, c_hist)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c_out, r_out) and _bits(c_gg, r_gg) and torch.equal(c_gx, r_gx)
    g.copy_(g2)   # new contents behind the captured pointers
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c_out, r2)
