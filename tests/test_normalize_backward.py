"""The backward of the normalisation: cspn2d_normalize_backward_f32, the differentiable cspn_amd.cspn2d_normalize and
train_utils.guidance_heads(..., norm_type='8sum' | '8sum_abs') under autograd.  Golden vectors: tests/golden/cspn2d_norm_grad_golden.npz (the
reference's affinity_normalization under autograd, make_norm_grad_golden.py) and tests/golden/head_norm_grad_golden.npz (reference heads ->
reference Affinity_Propagate under autograd, make_head_norm_grad_golden.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from helpers import assert_close, rel_err  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DY = [1, 1, 1, 0, 0, -1, -1, -1]   # cspn_common.h dy2 / dx2
DX = [1, 0, -1, 1, -1, 1, 0, -1]


def _cases(fname):
    z = np.load(os.path.join(GOLDEN, fname))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    return cases


NG = _cases("cspn2d_norm_grad_golden.npz")
HG = _cases("head_norm_grad_golden.npz")


def _norm_case(name):
    c = NG[name]
    g = c["guidance"] if "guidance" in c else np.load(os.path.join(GOLDEN, "cspn2d_golden.npz"))[name + "/guidance"]
    return g, c["grad_wb"], c["grad_guidance"], "8sum_abs" if int(c["meta"][0]) else "8sum"


def norm_grad_np(g, R, norm):
    """float64 restatement of include/cspn_amd.h cspn2d_normalize_backward_f32:
    dL/dg_k(p + off_k) = R_k(p) / S(p) - sign(G_k(p)) T(p) / S(p)^2  [* sign(g_k(p + off_k)) for 8sum_abs]; unread elements 0"""
    g, R = np.asarray(g, np.float64), np.asarray(R, np.float64)
    B, _, H, W = g.shape
    gt = np.abs(g) if norm == "8sum_abs" else g
    pad = np.pad(gt, ((0, 0), (0, 0), (1, 1), (1, 1)))
    G = np.stack([pad[:, k, 1 + DY[k]:1 + DY[k] + H, 1 + DX[k]:1 + DX[k] + W] for k in range(8)], 1)
    S = np.abs(G).sum(1, keepdims=True)
    T = (R * G).sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = R / S - np.sign(G) * T / (S * S)
    out = np.zeros((B, 8, H + 2, W + 2))
    for k in range(8):   # d_k(p) lands on g_k(p + off_k); what lands on the ring is read from the zero padding, not from g
        out[:, k, 1 + DY[k]:1 + DY[k] + H, 1 + DX[k]:1 + DX[k] + W] = d[:, k]
    out = out[:, :, 1:-1, 1:-1]
    return out * np.sign(g) if norm == "8sum_abs" else out


def unread_mask(B, H, W):
    m = np.zeros((B, 8, H, W), bool)
    y, x = np.mgrid[0:H, 0:W]
    for k in range(8):
        m[:, k] = ((y - DY[k] < 0) | (y - DY[k] >= H) | (x - DX[k] < 0) | (x - DX[k] >= W))[None]
    return m


def _golden_expected(ref, B, H, W):
    """the reference's dL/dguidance with its unread elements set to 0: the reference reads them only from the padding ring its crop
    discards, where R = 0 gives 0 / S = 0 -- or NaN where that ring pixel's S is 0 (make_norm_grad_golden.py); the engine writes 0"""
    un = unread_mask(B, H, W)
    assert np.all((ref[un] == 0) | np.isnan(ref[un]))
    e = ref.astype(np.float64).copy()
    e[un] = 0.0
    return e


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------

def test_header_declares_and_library_exports_normalize_backward():
    import cspn_amd
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    assert re.search(r"int\s+cspn2d_normalize_backward_f32\s*\(\s*const float\* guidance,\s*const float\* grad_wb,\s*float\* grad_guidance,"
                     r"\s*int B,\s*int H,\s*int W,\s*int norm_type,\s*cspn_stream_t stream\)", text)
    assert hasattr(cspn_amd.load(), "cspn2d_normalize_backward_f32")
    assert "cspn2d_normalize_backward" in cspn_amd.__all__


@pytest.mark.parametrize("name", sorted(NG))
def test_formula_reproduces_reference_autograd(name):
    """the float64 restatement of the kernel's formula against the unmodified reference under autograd"""
    g, R, ref, norm = _norm_case(name)
    B, _, H, W = g.shape
    got = norm_grad_np(g, R, norm)
    assert np.all(got[unread_mask(B, H, W)] == 0)
    assert_close(got, _golden_expected(ref, B, H, W), name, rtol=1e-5, atol_frac=1e-6)


def test_golden_set_covers_the_edge_cases():
    shapes = {n: _norm_case(n)[0].shape for n in NG}
    assert any(s[3] >= 256 for s in shapes.values())
    assert {_norm_case(n)[3] for n in NG} == {"8sum", "8sum_abs"}
    g, R, ref, _ = _norm_case("k_edge_zeros_8sum")
    assert (g == 0).any() and (g < 0).any() and np.isnan(ref[~unread_mask(1, *g.shape[2:])]).any()


@pytest.mark.parametrize("name", sorted(HG))
def test_head_norm_golden_vs_torch_fp64(name):
    """the pipeline golden (reference heads -> reference Affinity_Propagate, float32 autograd) against torch autograd in float64 through
    the plain-torch restatement (tools/torch_path.py): the golden is well conditioned enough to hold the engine to 2e-4"""
    import torch.nn.functional as F
    from tools.torch_path import cspn2d_torch
    c = HG[name]
    oh, ow, N, ab = map(int, c["meta"])
    x, w6, w5 = (torch.from_numpy(c[k]).double().requires_grad_(True) for k in ("x", "w6", "w5"))
    C = x.shape[1]
    up = torch.zeros(C, 1, 2, 2, dtype=torch.float64)
    up[:, :, 0, 0] = 1
    U = F.conv_transpose2d(x, up, stride=2, groups=C)[:, :, :oh, :ow]
    sp = torch.from_numpy(c["sparse"]).double() if "sparse" in c else None
    out = cspn2d_torch(F.conv2d(U, w6, padding=1), F.conv2d(U, w5, padding=1), sp, N, "8sum_abs" if ab else "8sum")
    (out * torch.from_numpy(c["grad_out"]).double()).sum().backward()
    for t, k in ((x, "grad_x"), (w6, "grad_w6"), (w5, "grad_w5")):
        assert rel_err(t.grad.numpy(), c[k]) <= 2e-5, k


def test_argument_errors_are_reported_without_gpu():
    import cspn_amd
    from cspn_amd import _lib
    f = _lib.late_symbol("cspn2d_normalize_backward_f32")
    a, b, o = 4096, 8192, 16384   # never dereferenced: every call below is rejected before a launch
    assert f(a, b, o, 1, 4, 4, 2, None) == -1   # NONE
    assert f(a, b, o, 1, 4, 4, 3, None) == -1   # PRENORM
    assert f(a, b, o, 1, 4, 4, 7, None) == -1
    assert b"norm_type" in cspn_amd.load().cspn_last_error()
    assert f(None, b, o, 1, 4, 4, 0, None) == -1 and f(a, None, o, 1, 4, 4, 0, None) == -1 and f(a, b, None, 1, 4, 4, 0, None) == -1
    assert f(a, b, o, 0, 4, 4, 0, None) == -1 and f(a, b, o, 1, 0, 4, 0, None) == -1 and f(a, b, o, 1, 4, -1, 0, None) == -1
    assert f(a, b, a, 1, 4, 4, 0, None) == -1 and f(a, b, b, 1, 4, 4, 1, None) == -1
    assert b"alias" in cspn_amd.load().cspn_last_error()


def test_stale_library_says_rebuild(monkeypatch):
    from cspn_amd import _lib
    monkeypatch.setitem(_lib._LATE_SYMBOLS, "cspn2d_not_exported_f32", (ctypes.c_int, []))
    with pytest.raises(_lib.CspnError, match="rebuild"):
        _lib.late_symbol("cspn2d_not_exported_f32")


def test_guidance_heads_normalised_training_checks_rank():
    from cspn_amd.train_utils import guidance_heads
    x = torch.zeros(4, 3, 3, requires_grad=True)
    with pytest.raises(ValueError, match="x must be"):
        guidance_heads(x, torch.zeros(8, 4, 3, 3), None, 0, 0, "8sum")
    with pytest.raises(ValueError, match="norm_type"):
        guidance_heads(torch.zeros(1, 4, 3, 3, requires_grad=True), torch.zeros(8, 4, 3, 3), None, 0, 0, "none")


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------

def _torch_fp64_grad(g, R, norm):
    """dL/dg by torch autograd in float64 through tools/torch_path._gather8(g~) / |.|.sum"""
    from tools.torch_path import _gather8
    gd = g.double().clone().requires_grad_(True)
    gt = gd.abs() if norm == "8sum_abs" else gd
    G = _gather8(gt)
    w = G / G.abs().sum(1, keepdim=True)
    w.backward(R.double())
    return gd.grad


def _inputs(B, H, W, seed, device="cuda"):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, 8, H, W, generator=gen)
    g[torch.rand(B, 8, H, W, generator=gen) < 0.1] = 0.0          # exact zeros (sign(0)); randn gives the negatives
    R = torch.randn(B, 8, H, W, generator=gen)
    return g.to(device), R.to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NG))
def test_kernel_vs_reference_golden(name):
    import cspn_amd
    g, R, ref, norm = _norm_case(name)
    B, _, H, W = g.shape
    got = cspn_amd.cspn2d_normalize_backward(torch.from_numpy(g).cuda(), torch.from_numpy(R).cuda(), norm).cpu().numpy()
    assert np.all(got[unread_mask(B, H, W)] == 0)   # unread elements: 0 (the reference's ring NaN / 0 there, see _golden_expected)
    assert_close(got, _golden_expected(ref, B, H, W), name, rtol=1e-5, atol_frac=1e-5)


_SIZES = [1, 2, 3, 7, 64, 255, 256, 257, 1216, 1218]
_FUZZ = [(1 + 2 * (i % 2), h, w) for i, (h, w) in enumerate(zip(_SIZES, _SIZES[::-1]))] + \
        [(1, h, h) for h in _SIZES[:8]] + [(3, 7, 1218), (1, 255, 257), (3, 64, 1216), (1, 1216, 7), (3, 2, 255)]


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("B,H,W", _FUZZ)
def test_kernel_fuzz_vs_torch_fp64(B, H, W, norm):
    import cspn_amd
    g, R = _inputs(B, H, W, seed=B * 7919 + H * 31 + W)
    got = cspn_amd.cspn2d_normalize_backward(g, R, norm)
    ref = _torch_fp64_grad(g, R, norm)
    assert_close(got.cpu().numpy(), ref.cpu().numpy(), "%dx%dx%d %s" % (B, H, W, norm), rtol=1e-5, atol_frac=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
def test_kernel_misaligned_views(norm):
    """inputs AND output as views offset by one float (4-byte aligned only), W % 4 != 0, through the C ABI"""
    import cspn_amd
    B, H, W = 2, 37, 259
    g, R = _inputs(B, H, W, seed=5)
    n = B * 8 * H * W
    bufs = [torch.zeros(n + 1, device="cuda") for _ in range(3)]
    gv, rv, ov = (b[1:].view(B, 8, H, W) for b in bufs)
    gv.copy_(g)
    rv.copy_(R)
    assert gv.data_ptr() % 16 == 4
    f = cspn_amd._lib.late_symbol("cspn2d_normalize_backward_f32")
    rc = f(gv.data_ptr(), rv.data_ptr(), ov.data_ptr(), B, H, W, 1 if norm == "8sum_abs" else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    ref = _torch_fp64_grad(g, R, norm)
    assert_close(ov.cpu().numpy(), ref.cpu().numpy(), "misaligned", rtol=1e-5, atol_frac=1e-5)
    assert float(bufs[2][0]) == 0.0   # nothing written before the view
    assert torch.equal(cspn_amd.cspn2d_normalize_backward(gv, rv, norm), ov)   # the Python entry point on misaligned inputs


@pytest.mark.gpu
def test_kernel_is_deterministic():
    import cspn_amd
    g, R = _inputs(3, 129, 1218, seed=9)
    for norm in ("8sum", "8sum_abs"):
        a = cspn_amd.cspn2d_normalize_backward(g, R, norm)
        b = cspn_amd.cspn2d_normalize_backward(g, R, norm)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
def test_consistent_with_raw_route(norm):
    """dL/dguidance of the raw route (cspn2d_backward with the normalisation chained inside) == the PRENORM backward's dL/dwb chained
    through cspn2d_normalize_backward"""
    import cspn_amd
    from helpers import make_inputs
    g, h, s = make_inputs(2, 64, 512, seed=21)
    g, h, s = g.cuda(), h.cuda(), s.cuda()
    go = torch.randn(2, 1, 64, 512, generator=torch.Generator().manual_seed(22)).cuda()
    ga, _ = cspn_amd.cspn2d_backward(g, h, s, go, 24, norm)
    gwb, _ = cspn_amd.cspn2d_backward(cspn_amd.cspn2d_normalize(g, norm), h, s, go, 24, "prenorm")
    gb = cspn_amd.cspn2d_normalize_backward(g, gwb, norm)
    assert rel_err(gb.cpu().numpy(), ga.cpu().numpy()) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
def test_normalize_autograd(norm):
    import cspn_amd
    from cspn_amd import _lib
    g, R = _inputs(2, 33, 70, seed=3)
    # grad off / no grad required: today's kernel, bit for bit, and no graph
    direct = torch.empty_like(g)
    assert _lib.load().cspn2d_normalize_f32(g.data_ptr(), direct.data_ptr(), 2, 33, 70, _lib.NORM_TYPES[norm],
                                            torch.cuda.current_stream().cuda_stream) == 0
    plain = cspn_amd.cspn2d_normalize(g, norm)
    ga = g.clone().requires_grad_(True)
    with torch.no_grad():
        nograd = cspn_amd.cspn2d_normalize(ga, norm)
    for t in (plain, nograd):
        assert t.grad_fn is None and torch.equal(t.view(torch.int32), direct.view(torch.int32))
    # grad on
    wb = cspn_amd.cspn2d_normalize(ga, norm)
    assert wb.grad_fn is not None and torch.equal(wb.detach().view(torch.int32), direct.view(torch.int32))
    wb.backward(R)
    assert_close(ga.grad.cpu().numpy(), _torch_fp64_grad(g, R, norm).cpu().numpy(), "autograd", rtol=1e-5, atol_frac=1e-5)


def _head_inputs(B, C, h, w, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=gen, device="cuda")
    w6 = torch.randn(8, C, 3, 3, generator=gen, device="cuda") / 12
    w5 = torch.randn(1, C, 3, 3, generator=gen, device="cuda") / 12 + 0.05
    return x, w6, w5


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
def test_guidance_heads_normalised_with_grad_matches_fused(norm):
    from cspn_amd.train_utils import guidance_heads
    x, w6, w5 = _head_inputs(2, 16, 9, 70, seed=4)
    with torch.no_grad():
        g0, b0 = guidance_heads(x, w6, w5, 17, 139, norm)
    xa = x.clone().requires_grad_(True)
    g1, b1 = guidance_heads(xa, w6, w5, 17, 139, norm)
    assert g1.grad_fn is not None and b1.grad_fn is not None and g0.grad_fn is None
    assert rel_err(g1.detach().cpu().numpy(), g0.cpu().numpy()) <= 1e-6
    assert rel_err(b1.detach().cpu().numpy(), b0.cpu().numpy()) <= 1e-6
    print("gate_wb with grad == fused gate_wb bitwise (%s): %s" % (norm, torch.equal(g1.detach().view(torch.int32), g0.view(torch.int32))))


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
def test_heads_norm_plus_prenorm_train_step(norm):
    """heads(norm) -> propagate_prenorm (training mode: kept checkpoints) -> loss.backward(): dL/dx, dL/dW6, dL/dW5 against torch fp64
    autograd through the reference's op sequence, and against the raw route's engine gradients (heads raw -> Affinity_Propagate(norm))"""
    import torch.nn.functional as F
    import cspn_amd
    from cspn_amd.train_utils import guidance_heads
    from tools.torch_path import cspn2d_torch
    B, C, h, w, N = 2, 16, 20, 140, 24
    x, w6, w5 = _head_inputs(B, C, h, w, seed=12)
    gen = torch.Generator(device="cuda").manual_seed(13)
    sp = (torch.rand(B, 1, 2 * h, 2 * w, generator=gen, device="cuda") < 0.03).float() * 2.0
    go = torch.randn(B, 1, 2 * h, 2 * w, generator=gen, device="cuda")
    assert cspn_amd.functional.cspn2d_history_bytes(B, 2 * h, 2 * w, N) > 0   # the training-mode forward really runs
    xa, w6a, w5a = (t.clone().requires_grad_(True) for t in (x, w6, w5))
    wb, b = guidance_heads(xa, w6a, w5a, 0, 0, norm)
    out = cspn_amd.propagate_prenorm(wb, b, sp, N)
    (out * go).sum().backward()
    xr, w6r, w5r = (t.clone().requires_grad_(True) for t in (x, w6, w5))
    g, b = guidance_heads(xr, w6r, w5r)
    outr = cspn_amd.Affinity_Propagate(N, 3, norm)(g, b, sp)
    (outr * go).sum().backward()
    xb, w6b, w5b = (t.double().clone().requires_grad_(True) for t in (x, w6, w5))
    up = torch.zeros(C, 1, 2, 2, device="cuda", dtype=torch.float64)
    up[:, :, 0, 0] = 1
    U = F.conv_transpose2d(xb, up, stride=2, groups=C)
    ref = cspn2d_torch(F.conv2d(U, w6b, padding=1), F.conv2d(U, w5b, padding=1), sp.double(), N, norm)
    (ref * go.double()).sum().backward()
    assert float((out.detach().double() - ref.detach()).abs().max() / ref.detach().abs().max()) <= 1e-5
    for a, r, e, what in ((xa.grad, xb.grad, xr.grad, "x"), (w6a.grad, w6b.grad, w6r.grad, "w6"), (w5a.grad, w5b.grad, w5r.grad, "w5")):
        assert float((a.double() - r).abs().max() / r.abs().max()) <= 2e-4, what
        assert float((a - e).abs().max() / e.abs().max()) <= 1e-4, what + " (raw route)"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HG))
def test_heads_norm_plus_prenorm_vs_reference_golden(name):
    import cspn_amd
    from cspn_amd.train_utils import guidance_heads
    c = HG[name]
    oh, ow, N, ab = map(int, c["meta"])
    x, w6, w5 = (torch.from_numpy(c[k]).cuda().requires_grad_(True) for k in ("x", "w6", "w5"))
    sp = torch.from_numpy(c["sparse"]).cuda() if "sparse" in c else None
    wb, b = guidance_heads(x, w6, w5, oh, ow, "8sum_abs" if ab else "8sum")
    out = cspn_amd.propagate_prenorm(wb, b, sp, N)
    (out * torch.from_numpy(c["grad_out"]).cuda()).sum().backward()
    assert rel_err(out.detach().cpu().numpy(), c["out"]) <= 1e-5
    for t, k in ((x, "grad_x"), (w6, "grad_w6"), (w5, "grad_w5")):
        assert rel_err(t.grad.cpu().numpy(), c[k]) <= 2e-4, k


@pytest.mark.gpu
def test_argument_checks_on_device():
    import cspn_amd
    lib = cspn_amd.load()
    f = cspn_amd._lib.late_symbol("cspn2d_normalize_backward_f32")
    g, R = _inputs(1, 5, 6, seed=1)
    o = torch.full_like(g, 7.0)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()   # noqa: E731
    for norm in (2, 3):                                          # NONE, PRENORM
        assert f(P(g), P(R), P(o), 1, 5, 6, norm, st) == -1
    assert f(None, P(R), P(o), 1, 5, 6, 0, st) == -1
    assert f(P(g), None, P(o), 1, 5, 6, 0, st) == -1
    assert f(P(g), P(R), None, 1, 5, 6, 0, st) == -1
    assert f(P(g), P(R), P(o), 1, 5, 0, 0, st) == -1             # a zero size
    assert f(P(g), P(R), P(g), 1, 5, 6, 0, st) == -1             # output aliases an input
    assert f(P(g), P(R), P(R), 1, 5, 6, 1, st) == -1
    assert lib.cspn_last_error()
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                # nothing was launched
    assert f(P(g), P(R), P(o), 1, 5, 6, 0, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o).all()) and not bool((o == 7.0).any())
