"""The guidance heads for 5x5 and 7x7 propagation on a float16 / bfloat16 feature map: cspn_guidance_head_kxk_g16 / cspn_guidance_head_kxk_backward_g16,
train_utils.guidance_heads with a 16-bit x and weight_guidance [24 | 48, C, 3, 3].  The reference is the float64 statement of tests/test_head_kxk.py evaluated on
the ROUNDED operands (x, the weights and dL/dblur rounded to dt; dL/dguidance is dt already), so what is measured is the engine's own error:
  * tensors stored in dt (guidance, dL/dx): |a - ref| <= 2^-p |ref| + 1e-5 max|ref|, p = 11 (float16) / 8 (bfloat16) -- the half ulp of the one rounding plus
    the float32-accumulation bound tests/test_head_kxk.py uses for these sums;
  * float32 outputs: blur <= 1e-5 of the plane maximum, dL/dW <= 2e-5, as tests/test_head_kxk.py."""
import os

import numpy as np
import pytest
import torch

from test_head_kxk import PLANES, _rel, statement_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = {"float16": (torch.float16, 11), "bfloat16": (torch.bfloat16, 8)}
NEW = ["cspn_guidance_head_kxk_g16_workspace_bytes", "cspn_guidance_head_kxk_g16", "cspn_guidance_head_kxk_backward_g16_workspace_bytes",
       "cspn_guidance_head_kxk_backward_g16"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_g16_symbols_are_declared_and_exported():
    from cspn_amd import _lib
    header = open(os.path.join(ROOT, "include", "cspn_amd.h")).read()
    for n in NEW:
        assert n in _lib._LATE_SYMBOLS and (n + "(") in header
    assert "#define CSPN_ABI_VERSION 5" in header


@pytest.mark.parametrize("dx,dw", [(torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16)])
def test_dtype_mismatch_is_a_type_error_on_cpu_tensors(dx, dw):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    x = torch.zeros(1, 4, 3, 3, dtype=dx)
    with pytest.raises(TypeError) as e:
        guidance_heads(x, torch.zeros(24, 4, 3, 3, dtype=dw))
    assert str(dx) in str(e.value) and str(dw) in str(e.value)
    with pytest.raises(TypeError) as e:
        guidance_heads(x, torch.zeros(48, 4, 3, 3), torch.zeros(1, 4, 3, 3, dtype=dw))
    assert str(dx) in str(e.value) and str(dw) in str(e.value)
    with pytest.raises(TypeError) as e:
        guidance_heads_backward(x, torch.zeros(24, 4, 3, 3, dtype=dw), None, torch.zeros(1, 24, 6, 6, dtype=dx), None)
    assert str(dx) in str(e.value) and str(dw) in str(e.value)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_16_bit_x_with_8_plane_weights_names_the_float32_only_head(dt):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    x = torch.zeros(1, 4, 3, 3, dtype=dt)
    with pytest.raises(TypeError, match="3 x 3 guidance head .* is float32 only"):
        guidance_heads(x, torch.zeros(8, 4, 3, 3))
    with pytest.raises(TypeError, match="3 x 3 guidance head .* is float32 only"):
        guidance_heads_backward(x, torch.zeros(8, 4, 3, 3), None, torch.zeros(1, 8, 6, 6), None)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _inputs(B, C, h, w, H, W, K, seed, dt, scale=None):
    """-> x (dt), wg, wb (float32 masters), gg (dt), gb (float32), on the GPU"""
    gen = torch.Generator().manual_seed(seed)
    P = PLANES[K]
    s = scale if scale is not None else 3.0 * C ** 0.5
    x = torch.randn(B, C, h, w, generator=gen)
    wg = torch.randn(P, C, 3, 3, generator=gen) / s
    wb = torch.randn(1, C, 3, 3, generator=gen) / s
    gg, gb = torch.randn(B, P, H, W, generator=gen), torch.randn(B, 1, H, W, generator=gen)
    return x.cuda().to(dt), wg.cuda(), wb.cuda(), gg.cuda().to(dt), gb.cuda()


def _reference(x, wg, wb, gg, gb, oh, ow):
    """the float64 statement on the rounded operands"""
    dt = x.dtype
    return statement_grads(x.double(), wg.to(dt).double(), wb.to(dt).double() if wb is not None else None, gg.double(),
                           gb.to(dt).double() if gb is not None else None, oh, ow)


def _err16(a, ref, p):
    """the largest |a - ref| / (2^-p |ref| + 1e-5 max|ref|): <= 1 is inside the bound"""
    a, ref = a.double(), ref.double()
    assert a.shape == ref.shape and bool(torch.isfinite(a).all())
    bound = 2.0 ** -p * ref.abs() + 1e-5 * max(1e-30, float(ref.abs().max()))
    return float(((a - ref).abs() / bound).max())


def _check_all(x, wg, wb, gg, gb, oh, ow, p, what):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    rg, rb, rdx, rdwg, rdwb = _reference(x, wg, wb, gg, gb, oh, ow)
    g, b = guidance_heads(x, wg, wb, oh, ow)
    dx, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb)
    torch.cuda.synchronize()
    assert g.dtype == x.dtype and dx.dtype == x.dtype and dwg.dtype == torch.float32
    e16 = {"guidance": _err16(g, rg, p), "dx": _err16(dx, rdx, p)}
    e32 = {"dwg": _rel(dwg, rdwg)}
    if wb is not None:
        assert b.dtype == torch.float32 and dwb.dtype == torch.float32
        e32["blur"], e32["dwb"] = _rel(b, rb), _rel(dwb, rdwb)
    else:
        assert b is None and dwb is None
    print(what, {k: "%.2f" % v for k, v in e16.items()}, {k: "%.2e" % v for k, v in e32.items()})
    for k, v in e16.items():
        assert v <= 1.0, (what, k, v)
    for k, v in e32.items():
        assert v <= (1e-5 if k == "blur" else 2e-5), (what, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_engine_fuzzed_small_shapes(dtn, K):
    """seeded small shapes: 1 .. 3 images, heights 1 .. 9, C below, at and above the 8- and 16-deep k blocks, widths below, at and above the 32-column and
    16-pixel tiles; exact 2x and narrowed outputs incl. odd sizes; with and without the blur head"""
    dt, p = DTS[dtn]
    rng = np.random.default_rng(1600 + K)
    for case in range(24):
        B, C = int(rng.integers(1, 4)), int(rng.choice([1, 7, 8, 15, 16, 17, 33, 64]))
        h = int(rng.integers(1, 10))
        w = int(rng.choice([1, 2, 3, 7, 9, 31, 32, 33, 65]))
        oh, ow = 0, 0
        if rng.random() < 0.6:
            oh, ow = int(rng.integers(max(1, 2 * h - 3), 2 * h + 1)), int(rng.integers(max(1, 2 * w - 3), 2 * w + 1))
        H, W = (oh, ow) if oh else (2 * h, 2 * w)
        x, wg, wb, gg, gb = _inputs(B, C, h, w, H, W, K, 1600 * K + case, dt, scale=3.0)
        if case % 4 == 3:
            wb, gb = None, None
        _check_all(x, wg, wb, gg, gb, oh, ow, p, "%s K%d case %d: B%d C%d h%d w%d -> %dx%d" % (dtn, K, case, B, C, h, w, H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_engine_at_one_reference_sized_row(dtn, K):
    dt, p = DTS[dtn]
    _check_all(*_inputs(1, 64, 152, 608, 304, 1216, K, 760 + K, dt), 0, 0, p, "%s K%d 1x64x152x608" % (dtn, K))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_two_byte_aligned_views_and_odd_width_take_the_guarded_path(dtn, K):
    """x and dL/dguidance as contiguous views one element into their buffers (2-byte aligned, not 4), and an odd output width"""
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    dt, p = DTS[dtn]
    for (B, C, h, w, oh, ow) in ((2, 17, 5, 33, 0, 0), (1, 16, 6, 40, 11, 79)):
        H, W = (oh, ow) if oh else (2 * h, 2 * w)
        x, wg, wb, gg, gb = _inputs(B, C, h, w, H, W, K, 40 + K + w, dt)
        xv = torch.empty(x.numel() + 1, dtype=dt, device="cuda")[1:].view_as(x).copy_(x)
        gv = torch.empty(gg.numel() + 1, dtype=dt, device="cuda")[1:].view_as(gg).copy_(gg)
        assert xv.data_ptr() % 4 == 2 and gv.data_ptr() % 4 == 2 and xv.is_contiguous() and gv.is_contiguous()
        _check_all(xv, wg, wb, gv, gb, oh, ow, p, "%s K%d views %dx%d -> %dx%d" % (dtn, K, h, w, H, W))
        g0, b0 = guidance_heads(x, wg, wb, oh, ow)
        g1, b1 = guidance_heads(xv, wg, wb, oh, ow)
        assert torch.equal(g0, g1) and torch.equal(b0, b1)
        for a, r in zip(guidance_heads_backward(xv, wg, wb, gv, gb), guidance_heads_backward(x, wg, wb, gg, gb)):
            assert torch.equal(a, r)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_backward_is_deterministic_and_subsets_return_none(dtn, K):
    from cspn_amd.train_utils import guidance_heads_backward
    dt, p = DTS[dtn]
    x, wg, wb, gg, gb = _inputs(2, 64, 37, 150, 73, 299, K, 9 + K, dt)
    a = guidance_heads_backward(x, wg, wb, gg, gb)
    b = guidance_heads_backward(x, wg, wb, gg, gb)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    dx, n1, n2 = guidance_heads_backward(x, wg, wb, gg, gb, need_w=False)
    assert n1 is None and n2 is None and torch.equal(dx, a[0])
    n0, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb, need_x=False)
    assert n0 is None and torch.equal(dwg, a[1]) and torch.equal(dwb, a[2])
    assert all(t is None for t in guidance_heads_backward(x, wg, wb, gg, gb, need_x=False, need_w=False))
    dx2, dwg2, none = guidance_heads_backward(x, wg, None, gg, None)                # guidance head only
    r = _reference(x, wg, None, gg, None, 73, 299)
    assert none is None and _err16(dx2, r[2], p) <= 1.0 and _rel(dwg2, r[3]) <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_autograd_train_step_is_the_manual_composition(dtn):
    """guidance_heads(x16, wg, wb) -> Affinity_PropagateKxK(12, 5, '8sum') with a sparse mask -> loss.backward() against cspn2d_backward_kxk_norm ->
    guidance_heads_backward, bitwise; the dtypes of every tensor on the way; 16-bit weights get the float32 gradients .to(dt)"""
    import cspn_amd
    from cspn_amd.functional import cspn2d_backward_kxk_norm
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    dt, _ = DTS[dtn]
    B, C, h, w, N, K = 2, 16, 20, 70, 12, 5
    gen = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(B, C, h, w, generator=gen, device="cuda").to(dt)
    wg = torch.randn(24, C, 3, 3, generator=gen, device="cuda") / 12
    wb = torch.randn(1, C, 3, 3, generator=gen, device="cuda") / 12 + 0.05
    sp = (torch.rand(B, 1, 2 * h, 2 * w, generator=gen, device="cuda") < 0.03).float() * 2.0
    go = torch.randn(B, 1, 2 * h, 2 * w, generator=gen, device="cuda")
    xa, wga, wba = (t.clone().requires_grad_(True) for t in (x, wg, wb))
    g, b = guidance_heads(xa, wga, wba)
    assert g.grad_fn is not None and g.grad_fn is b.grad_fn                       # one autograd Function for both heads
    assert g.dtype == dt and b.dtype == torch.float32
    out = cspn_amd.Affinity_PropagateKxK(N, K, "8sum")(g, b, sp)
    (out * go).sum().backward()
    assert xa.grad.dtype == dt and wga.grad.dtype == torch.float32 and wba.grad.dtype == torch.float32
    gg, gb = cspn2d_backward_kxk_norm(g.detach(), b.detach(), sp, go, K, N, "8sum")
    assert gg.dtype == dt and gb.dtype == torch.float32
    dx, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb)
    assert torch.equal(xa.grad, dx) and torch.equal(wga.grad, dwg) and torch.equal(wba.grad, dwb)
    # weights that are dt themselves: the same call on .float() (exact), their gradients .to(dt)
    xc, wgc, wbc = x.clone().requires_grad_(True), wg.to(dt).requires_grad_(True), wb.to(dt).requires_grad_(True)
    g2, b2 = guidance_heads(xc, wgc, wbc)
    assert torch.equal(g2, g) and torch.equal(b2, b)                              # (the engine rounds the masters to the same values)
    ((g2.float() * gg.float()).sum() + (b2 * gb).sum()).backward()
    assert wgc.grad.dtype == dt and wbc.grad.dtype == dt
    assert torch.equal(wgc.grad, dwg.to(dt)) and torch.equal(wbc.grad, dwb.to(dt)) and torch.equal(xc.grad, dx)
    # one head's gradient missing: zeros of the right dtype
    xd = x.clone().requires_grad_(True)
    g3, b3 = guidance_heads(xd, wg, wb)
    (b3 * gb).sum().backward()
    assert torch.equal(xd.grad, guidance_heads_backward(x, wg, wb, torch.zeros_like(gg), gb, need_w=False)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_float32_path_is_untouched(K):
    """guidance_heads on float32 inputs is bitwise cspn_guidance_head_kxk_f32 called through _lib directly"""
    from cspn_amd import _lib
    from cspn_amd.train_utils import guidance_heads
    B, C, h, w, H, W = 2, 33, 9, 70, 17, 139
    gen = torch.Generator().manual_seed(32 + K)
    x, wg, wb = (torch.randn(*s, generator=gen).cuda() for s in ((B, C, h, w), (PLANES[K], C, 3, 3), (1, C, 3, 3)))
    g, b = guidance_heads(x, wg, wb, H, W)
    rg, rb = torch.empty_like(g), torch.empty_like(b)
    n = _lib.late_symbol("cspn_guidance_head_kxk_workspace_bytes")(B, C, h, w, K)
    ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rc = _lib.late_symbol("cspn_guidance_head_kxk_f32")(x.data_ptr(), wg.data_ptr(), wb.data_ptr(), rg.data_ptr(), rb.data_ptr(), B, C, h, w, H, W, K,
                                                        ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and g.dtype == torch.float32 and torch.equal(g, rg) and torch.equal(b, rb)


@pytest.mark.gpu
def test_return_codes():
    from cspn_amd import _lib
    fwd_n, fwd, bwd_n, bwd = (_lib.late_symbol(n) for n in NEW)
    BADARG, WORKSPACE = -1, -2
    F16, BF16 = _lib.DTYPES["float16"], _lib.DTYPES["bfloat16"]
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()   # noqa: E731
    x = torch.zeros(1, 4, 3, 3, device="cuda", dtype=torch.float16)
    w24, w5 = torch.zeros(24, 4, 3, 3, device="cuda"), torch.zeros(1, 4, 3, 3, device="cuda")
    g, b = torch.zeros(1, 24, 6, 6, device="cuda", dtype=torch.float16), torch.zeros(1, 1, 6, 6, device="cuda")
    n = fwd_n(1, 4, 3, 3, 5)
    assert n > 0 and fwd_n(1, 4, 3, 3, 3) == 0 and fwd_n(1, 4, 3, 3, 4) == 0
    ws = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    assert fwd(P(x), F16, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == 0
    assert fwd(P(x), BF16, P(w24), None, P(g), None, 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == 0               # no blur head
    assert fwd(P(x), F16, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 3, P(ws), n, st) == BADARG          # K = 3: float32 only
    for bad in (0, 3):
        assert fwd(P(x), bad, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG      # dtype
    assert fwd(None, F16, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG
    assert fwd(P(x), F16, None, P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG
    assert fwd(P(x), F16, P(w24), P(w5), None, P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG
    assert fwd(P(x) + 1, F16, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG      # not 2-byte aligned
    assert fwd(P(x), F16, P(w24), P(w5), P(g), None, 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG          # w_blur without blur_out
    assert fwd(P(x), F16, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 7, 6, 5, P(ws), n, st) == BADARG          # H > 2 h
    assert fwd(P(x), F16, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n - 1, st) == WORKSPACE   # too small
    assert fwd(P(x), F16, P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws) + 8, n, st) == WORKSPACE   # misaligned
    dx, dwg, dwb = torch.empty_like(x), torch.empty_like(w24), torch.empty_like(w5)
    n = bwd_n(1, 4, 3, 3, 5)
    assert n > 0 and bwd_n(0, 4, 3, 3, 5) == 0 and bwd_n(1, 4, 3, 3, 3) == 0
    ws = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    assert bwd(P(x), F16, P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == 0
    assert bwd(P(x), F16, P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 3, P(ws), n, st) == BADARG
    for bad in (0, 3):
        assert bwd(P(x), bad, P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG
    assert bwd(P(x), F16, P(w24), P(w5), None, P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG
    assert bwd(P(x), F16, P(w24), P(w5), P(g) + 1, P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG
    assert bwd(P(x), F16, P(w24), P(w5), P(g), None, P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG   # a blur head without its gradient
    assert bwd(P(x), F16, P(w24), None, P(g), None, P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG    # grad_w_blur without a blur head
    assert bwd(P(x), F16, P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), 64, st) == WORKSPACE
    assert bwd(P(x), F16, P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws) + 8, n, st) == WORKSPACE
    assert bwd(P(x), F16, P(w24), P(w5), P(g), P(b), None, None, None, 1, 4, 3, 3, 6, 6, 5, None, 0, st) == 0              # nothing asked for
    torch.cuda.synchronize()
