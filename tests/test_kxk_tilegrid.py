"""The 2D K x K engine (cspn_amd/csrc/cspn2d_kxk.hip) on tile grids that are not square.  Every kernel there runs one 64 x 16 pixel tile
per workgroup, decodes (tile column, tile row, image) from a flat block index and stages an R-wide halo; on a square grid a swap of the two
tile counts is invisible, on a 2 x 2 grid no tile has neighbours on both sides, and a gradient that fits one tile never reads a halo.
The shapes below have 3 x 4, 5 x 2 and 2 x 5 tiles (rows x columns), interior tiles, last tiles no wider or taller than the halo of
K = 7, W % 4 in {0, 2, 3}, and two images, so that the image index is decoded on a non-square grid.
  1. the NONE op, forward, every kept level and both gradients against the float64 statement of test_kernel_size
  2. the depth-completion contract, K = 3 / 5 / 7, a mask per channel (the N' = B C view, cpg = C) and a shared one, against the float64
     statement of test_kxk_norm
  3. impulses at the corners of an interior seam and in the thin last tiles: the response against the statement, its support, and every
     other (image, channel) plane exactly zero
  4. <forward(x), y> == <x, backward_x(y)>, which ties the step to its adjoint without the torch statement
Tolerances are the project's: 1e-4 of max|ref| forward, helpers.assert_close(rtol=2e-4, atol_frac=5e-6) for gradients.  Each check prints
its error as a fraction of its bound before it asserts."""
import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import functional as F
from helpers import assert_close
from test_kernel_size import _gates, _torch_noneKxK, _values
from test_kxk_norm import _inputs, torch_kxk_norm

RTOL = 1e-4
GTOL, GFLOOR = 2e-4, 5e-6
ATOL_ADJ = 2e-4   # of sum |forward(x) y|: the gradient tolerance
# (H, W): tiles are 16 rows x 64 columns
SHAPES = {"wide": (35, 196),    # 3 x 4 tiles, W % 4 == 0 (the vector path), last tile column 4 px, last tile row 3 rows
          "tall": (67, 70),     # 5 x 2 tiles, W % 4 == 2 (the guarded path), last tile column 6 px, last tile row 3 rows
          "strip": (18, 259)}   # 2 x 5 tiles, W % 4 == 3, last tile column 3 px
NAMES = list(SHAPES)
N = 2


def _fwd(a, ref, what):
    """max|a - ref| <= RTOL max|ref|"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    e = float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))
    print("tilegrid fwd  %-40s %.3g of %g" % (what, e / RTOL, RTOL))
    assert np.isfinite(a).all() and e <= RTOL, "%s: relative error %.3g > %g" % (what, e, RTOL)


def _grad(a, ref, what):
    """helpers.assert_close(rtol=2e-4, atol_frac=5e-6); the figure printed is the worst |a - ref| / (GFLOOR max|ref| + GTOL |ref|)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    bound = GFLOOR * max(np.abs(ref).max(), 1e-30) + GTOL * np.abs(ref)
    print("tilegrid grad %-40s %.3g of the bound" % (what, float((np.abs(a - ref) / bound).max())))
    assert_close(a, ref, what, rtol=GTOL, atol_frac=GFLOOR)


def _levels(g, x, K, n):
    """H_1 .. H_n of the float64 statement"""
    out = []
    for _ in range(n):
        x = _torch_noneKxK(g, x, K, 1)
        out.append(x)
    return out


# ---- 1. the NONE op ----
@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("name", NAMES)
def test_none_op_forward_levels_and_gradients_vs_fp64(name, K):
    (H, W), C, n = SHAPES[name], 2, 3
    g = _gates(N, K, H, W, seed=K * 1000 + W)
    x = _values(N, C, H, W, seed=H + K)
    go = _values(N, C, H, W, seed=7 + W)
    gt, xt = g.double().requires_grad_(True), x.double().requires_grad_(True)
    lv = _levels(gt, xt, K, n)
    lv[-1].backward(go.double())
    gd, xd, god = g.cuda(), x.cuda(), go.cuda()
    out = F.cspn2d_forward_kxk(gd, xd, K, n)
    _fwd(out.cpu(), lv[-1].detach(), "none %s K=%d" % (name, K))
    out_h, hist = F.cspn2d_forward_kxk(gd, xd, K, n, return_history=True)
    assert torch.equal(out_h, out)
    kept = hist.view(n - 1, N, C, H, W)
    for t in range(n - 1):
        _fwd(kept[t].cpu(), lv[t].detach(), "none %s K=%d level %d" % (name, K, t + 1))
    gg, gx = F.cspn2d_backward_kxk(gd, xd, god, K, n)
    _grad(gg.cpu(), gt.grad, "none %s K=%d dL/dgate" % (name, K))   # summed over the C channels
    _grad(gx.cpu(), xt.grad, "none %s K=%d dL/dx" % (name, K))
    gg_h, gx_h = F.cspn2d_backward_kxk(gd, xd, god, K, n, hist)
    _grad(gg_h.cpu(), gt.grad, "none %s K=%d dL/dgate, kept history" % (name, K))
    _grad(gx_h.cpu(), xt.grad, "none %s K=%d dL/dx, kept history" % (name, K))
    gg2, gx2 = F.cspn2d_backward_kxk(gd, xd, god, K, n)
    assert torch.equal(gg2, gg) and torch.equal(gx2, gx), "the backward is not deterministic"
    assert torch.equal(gg_h, gg) and torch.equal(gx_h, gx), "the kept history gives other gradients than the recomputed one"


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_affinity_propagate_under_autograd_on_the_wide_grid(K):
    (H, W), C, n = SHAPES["wide"], 3, 3
    g = _gates(N, K, H, W, seed=K * 31)
    x = _values(N, C, H, W, seed=K)
    go = _values(N, C, H, W, seed=13)
    gt, xt = g.double().requires_grad_(True), x.double().requires_grad_(True)
    ref = _torch_noneKxK(gt, xt, K, n)
    (ref * go.double()).sum().backward()
    gc, xc = g.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    y = cspn_amd.affinity_propagate(xc, gc, kernel_size=K, n_iter=n)
    assert y.grad_fn is not None
    _fwd(y.detach().cpu(), ref.detach(), "affinity_propagate K=%d" % K)
    (y * go.cuda()).sum().backward()
    _grad(gc.grad.cpu(), gt.grad, "affinity_propagate K=%d dL/dgate_weight" % K)
    _grad(xc.grad.cpu(), xt.grad, "affinity_propagate K=%d dL/dinput" % K)


# ---- 2. the depth-completion contract ----
NORM_CASES = [(name, 2, "per") for name in NAMES] + [("wide", 3, "shared")]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("name,C,sparse", NORM_CASES)
def test_norm_contract_forward_and_gradients_vs_fp64(name, C, sparse, norm, K):
    (H, W), B, n = SHAPES[name], 2, 3
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K * 1000 + W * 10 + C)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(K + H))
    gt, ht, st = g.double().requires_grad_(True), h.double().requires_grad_(True), s.double()
    ref = torch_kxk_norm(gt, ht, st, K, n, norm)
    ref.backward(go.double())
    what = "norm %s %s %s K=%d" % (name, sparse, norm, K)
    gd, hd, sd, god = g.cuda(), h.cuda(), s.cuda(), go.cuda()
    out, hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, return_history=True)
    _fwd(out.cpu(), ref.detach(), what)
    assert torch.equal(F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm), out)
    kept = hist.view(n - 1, B, C, H, W)
    with torch.no_grad():
        for t in range(1, n):
            _fwd(kept[t - 1].cpu(), torch_kxk_norm(gt, ht, st, K, t, norm), what + " level %d" % t)
    gg, gh = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm)
    _grad(gg.cpu(), gt.grad, what + " dL/dguidance")
    _grad(gh.cpu(), ht.grad, what + " dL/dblur")
    gg_h, gh_h = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, hist)
    assert torch.equal(gg_h, gg) and torch.equal(gh_h, gh), "the kept history gives other gradients than the recomputed one"


# ---- 3. impulses ----
# the four pixels around an interior seam corner of the wide grid, the last pixel of the image (3-row last tile row, 4 px last tile
# column) and the first pixel of that last tile column in the first tile row
PROBES = [(15, 63), (15, 64), (16, 63), (16, 64), (34, 195), (2, 192)]


def _check_impulse(res, ref, py, px, reach, what):
    """res [N,C,H,W] from an impulse at (1, 1, py, px): the plane (1, 1) against ref within RTOL of its own maximum, nothing outside the
    (2 reach + 1)-wide box, and every other plane exactly zero (0 times a finite gate summed stays 0; -0.0 == 0)"""
    for i in range(res.shape[0]):
        for c in range(res.shape[1]):
            if (i, c) != (1, 1):
                bad = int((~(res[i, c] == 0)).sum())
                assert bad == 0, "%s: %d elements of image %d channel %d are not zero: the impulse of image 1 channel 1 leaked" % (what, bad, i, c)
    plane = res[1, 1]
    assert float(plane.abs().max()) > 0, what + ": no response"
    _fwd(plane, ref[1, 1], what)
    outside = plane.clone()
    outside[max(py - reach, 0):py + reach + 1, max(px - reach, 0):px + reach + 1] = 0
    bad = outside.nonzero()
    assert bad.numel() == 0, "%s: response outside the box of reach %d, first at %s" % (what, reach, bad[0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_forward_impulse_at_the_seam_corners(K):
    (H, W), C, n = SHAPES["wide"], 2, 2
    g = _gates(N, K, H, W, seed=K + 50)
    gd = g.cuda()
    for py, px in PROBES:
        x = torch.zeros(N, C, H, W)
        x[1, 1, py, px] = 1.0
        out = F.cspn2d_forward_kxk(gd, x.cuda(), K, n).cpu()
        ref = _torch_noneKxK(g.double(), x.double(), K, n)
        _check_impulse(out, ref, py, px, n * (K // 2), "impulse K=%d at (%d, %d) forward" % (K, py, px))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_backward_impulse_at_the_seam_corners(K):
    (H, W), C, n = SHAPES["wide"], 2, 2
    g = _gates(N, K, H, W, seed=K + 60)
    gd = g.cuda()
    xd = _values(N, C, H, W, seed=K).cuda()   # dL/dx does not depend on it
    for py, px in PROBES:
        go = torch.zeros(N, C, H, W)
        go[1, 1, py, px] = 1.0
        none, gx = F.cspn2d_backward_kxk(gd, xd, go.cuda(), K, n, need_gate=False)
        assert none is None
        xt = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
        _torch_noneKxK(g.double(), xt, K, n).backward(go.double())
        _check_impulse(gx.cpu(), xt.grad, py, px, n * (K // 2), "impulse K=%d at (%d, %d) dL/dx" % (K, py, px))


# ---- 4. adjointness ----
def _dot(a, b):
    return float((a.double().cpu() * b.double().cpu()).sum())


def _adjoint(fx, y, x, bty, what):
    """<fx, y> == <x, bty> within ATOL_ADJ sum |fx y|, all three sums in float64 on the host"""
    lhs, rhs = _dot(fx, y), _dot(x, bty)
    scale = float((fx.double().cpu() * y.double().cpu()).abs().sum())
    print("tilegrid adj  %-40s %.3g of the bound" % (what, abs(lhs - rhs) / (ATOL_ADJ * scale)))
    assert np.isfinite(lhs) and np.isfinite(rhs) and scale > 0
    assert abs(lhs - rhs) <= ATOL_ADJ * scale, "%s: <F x, y> = %.9g, <x, F^T y> = %.9g, sum |F x y| = %.6g" % (what, lhs, rhs, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("name", ["tall", "strip"])
def test_none_op_step_and_adjoint_step_are_adjoint(name, K, n):
    (H, W), C = SHAPES[name], 2
    g = _gates(N, K, H, W, seed=K * 7 + n).cuda()
    x = _values(N, C, H, W, seed=W + n).cuda()
    y = _values(N, C, H, W, seed=H + n).cuda()
    out = F.cspn2d_forward_kxk(g, x, K, n)
    none, bty = F.cspn2d_backward_kxk(g, x, y, K, n, need_gate=False)
    _adjoint(out, y, x, bty, "none %s K=%d n=%d" % (name, K, n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("name", ["tall", "strip"])
def test_norm_contract_and_its_blur_gradient_are_adjoint(name, norm, K, n):
    """without a mask; the map from blur to out is affine in general, so the inner products are taken on the difference of two inputs"""
    (H, W), B, C = SHAPES[name], 2, 2
    g, h1, _ = _inputs(B, C, H, W, K, None, seed=K * 11 + n)
    h2 = _inputs(B, C, H, W, K, None, seed=K * 13 + n)[1]
    y = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(W + K))
    gd, h1d, h2d, yd = g.cuda(), h1.cuda(), h2.cuda(), y.cuda()
    d = F.cspn2d_forward_kxk_norm(gd, h1d, None, K, n, norm).double() - F.cspn2d_forward_kxk_norm(gd, h2d, None, K, n, norm).double()
    none, bty = F.cspn2d_backward_kxk_norm(gd, h1d, None, yd, K, n, norm, need_guidance=False)
    assert none is None
    _adjoint(d, yd, h1d.double() - h2d.double(), bty, "norm %s %s K=%d n=%d" % (name, norm, K, n))
