"""The 3 x 3 model's guidance heads on a float16 / bfloat16 feature map, feeding the float32 ring: cspn_guidance_head_g16 / cspn_guidance_head_backward_g16,
train_utils.guidance_heads(..., guidance_dtype=torch.float32) and cspn_amd.GuidanceHeads.  The reference is the float64 statement of tests/test_head_kxk.py
(torch's Unpool + narrow + 3 x 3 conv and its autograd) evaluated on the ROUNDED operands -- x as given, the weights, dL/dguidance and dL/dblur rounded to dt --
so what is measured is the engine's own error, with the bounds of tests/test_head_kxk_g16.py:
  * float32 outputs (the unrounded accumulators): guidance and blur <= 1e-5 of the tensor's maximum, dL/dW <= 2e-5;
  * dL/dx, stored in dt: |a - ref| <= 2^-p |ref| + 1e-5 max|ref|, p = 11 (float16) / 8 (bfloat16): the half ulp of its one rounding plus the float32 sums."""
import ctypes
import os
import types

import pytest
import torch

from test_head_kxk import _rel, statement_grads
from test_head_kxk_g16 import DTS, _err16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn_guidance_head_g16_workspace_bytes", "cspn_guidance_head_g16", "cspn_guidance_head_backward_g16_workspace_bytes", "cspn_guidance_head_backward_g16"]
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_symbols_are_declared_and_exported_and_the_abi_version_stays():
    from cspn_amd import _lib
    header = open(os.path.join(ROOT, "include", "cspn_amd.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in _lib._SYMBOLS and (n + "(") in header and hasattr(lib, n)
    assert "#define CSPN_ABI_VERSION 5" in header and lib.cspn_abi_version() == 5 and _lib.ABI_VERSION == 5


@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("blur", [True, False])
def test_module_owns_the_two_weights(K, blur):
    import cspn_amd
    m = cspn_amd.GuidanceHeads(6, K, 11, 13, blur=blur)
    assert "GuidanceHeads" in cspn_amd.__all__ and isinstance(m, torch.nn.Module)
    assert tuple(m.weight_guidance.shape) == (K * K - 1, 6, 3, 3) and m.weight_guidance.dtype == F32 and m.weight_guidance.requires_grad
    assert list(m.state_dict()) == (["weight_guidance", "weight_blur"] if blur else ["weight_guidance"])
    assert [n for n, _ in m.named_parameters()] == list(m.state_dict())
    if blur:
        assert tuple(m.weight_blur.shape) == (1, 6, 3, 3) and m.weight_blur.dtype == F32
    else:
        assert m.weight_blur is None
    bound = 1.0 / (6 * 9) ** 0.5                        # nn.Conv2d's kaiming_uniform_(a = sqrt 5): uniform in +-1 / sqrt(fan_in)
    assert float(m.weight_guidance.detach().abs().max()) <= bound and float(m.weight_guidance.detach().abs().max()) > 0.5 * bound
    assert (m.oheight, m.owidth, m.in_channels, m.prop_kernel) == (11, 13, 6, K)
    with pytest.raises(ValueError):
        cspn_amd.GuidanceHeads(6, 4)


def _stand_in(planes, C, oh, ow, seed):
    w = torch.randn(planes, C, 3, 3, generator=torch.Generator().manual_seed(seed))
    return types.SimpleNamespace(conv1=types.SimpleNamespace(weight=w), oheight=oh, owidth=ow)


@pytest.mark.parametrize("planes", [8, 24, 48])
def test_from_reference_copies_weights_and_output_sizes(planes):
    import cspn_amd
    l6, l5 = _stand_in(planes, 5, 228, 304, 1), _stand_in(1, 5, 228, 304, 2)
    m = cspn_amd.GuidanceHeads.from_reference(l6, l5)
    assert m.prop_kernel == {8: 3, 24: 5, 48: 7}[planes] and (m.in_channels, m.oheight, m.owidth) == (5, 228, 304)
    assert torch.equal(m.weight_guidance, l6.conv1.weight) and torch.equal(m.weight_blur, l5.conv1.weight)
    assert m.weight_guidance.data_ptr() != l6.conv1.weight.data_ptr()              # copies
    m1 = cspn_amd.GuidanceHeads.from_reference(l6)
    assert m1.weight_blur is None and list(m1.state_dict()) == ["weight_guidance"]
    with pytest.raises(ValueError):
        cspn_amd.GuidanceHeads.from_reference(l6, _stand_in(1, 5, 228, 300, 3))
    with pytest.raises(ValueError):
        cspn_amd.GuidanceHeads.from_reference(_stand_in(9, 5, 0, 0, 4))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_default_arguments_behave_as_before_and_a_misused_guidance_dtype_is_a_value_error(dt):
    """on CPU tensors: every one of these is raised before any device check"""
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    x, x32 = torch.zeros(1, 4, 3, 3, dtype=dt), torch.zeros(1, 4, 3, 3)
    w8, w24, w1 = torch.zeros(8, 4, 3, 3), torch.zeros(24, 4, 3, 3), torch.zeros(1, 4, 3, 3)
    g8, g24, g1 = torch.zeros(1, 8, 6, 6), torch.zeros(1, 24, 6, 6, dtype=dt), torch.zeros(1, 1, 6, 6)
    with pytest.raises(TypeError, match="3 x 3 guidance head .* is float32 only"):
        guidance_heads(x, w8)
    with pytest.raises(TypeError, match="3 x 3 guidance head .* is float32 only"):
        guidance_heads(x, w8, w1, guidance_dtype=None)
    with pytest.raises(TypeError, match="3 x 3 guidance head .* is float32 only"):
        guidance_heads_backward(x, w8, None, g8, None)
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    for bad in (dict(weight_guidance=w24), dict(x=x32), dict(guidance_dtype=dt), dict(guidance_dtype=torch.float64), dict(norm_type="8sum"),
                dict(norm_type="8sum_abs")):
        kw = dict(x=x, weight_guidance=w8, weight_blur=w1, guidance_dtype=F32)
        kw.update(bad)
        with pytest.raises(ValueError):
            guidance_heads(**kw)
    for bad in (dict(weight_guidance=w24, grad_guidance=g24), dict(x=x32), dict(guidance_dtype=dt)):
        kw = dict(x=x, weight_guidance=w8, weight_blur=w1, grad_guidance=g8, grad_blur=g1, guidance_dtype=F32)
        kw.update(bad)
        with pytest.raises(ValueError):
            guidance_heads_backward(**kw)
    with pytest.raises(TypeError) as e:
        guidance_heads(x, w8.to(other), w1, guidance_dtype=F32)
    assert str(dt) in str(e.value) and str(other) in str(e.value)
    with pytest.raises(TypeError) as e:
        guidance_heads_backward(x, w8, w1.to(other), g8, g1, guidance_dtype=F32)
    assert str(dt) in str(e.value) and str(other) in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- GPU
SHAPES = [(1, 4, 1, 1, 2, 2),            # C below one k step, a single pixel
          (2, 20, 3, 5, 5, 9),           # C no multiple of 16, narrowed, odd W: the guarded stores
          (1, 64, 2, 33, 4, 66),         # crosses a 32-column segment, W % 4 != 0
          (1, 64, 3, 70, 6, 140),        # three segments, W % 4 == 0: the fast stores
          (1, 16, 4, 8, 7, 16),          # the last output row dropped
          (1, 64, 2, 152, 4, 304)]       # a reference-sized row pair
_CACHE = {}


def _case(shape, dtn, seed=0):
    """-> x (dt), wg, wb (float32 masters), gg, gb (float32) on the GPU, and the float64 statement on the rounded operands; computed once, never written to"""
    key = (shape, dtn, seed)
    if key not in _CACHE:
        B, C, h, w, H, W = shape
        dt = DTS[dtn][0]
        gen = torch.Generator().manual_seed(1000 * seed + 17 * C + w + (dt == torch.bfloat16))
        s = 3.0 * C ** 0.5
        x = torch.randn(B, C, h, w, generator=gen).cuda().to(dt)
        wg, wb = (torch.randn(8, C, 3, 3, generator=gen) / s).cuda(), (torch.randn(1, C, 3, 3, generator=gen) / s).cuda()
        gg, gb = torch.randn(B, 8, H, W, generator=gen).cuda(), torch.randn(B, 1, H, W, generator=gen).cuda()
        ref = statement_grads(x.double(), wg.to(dt).double(), wb.to(dt).double(), gg.to(dt).double(), gb.to(dt).double(), H, W)
        _CACHE[key] = (x, wg, wb, gg, gb, ref)
    return _CACHE[key]


def _check(x, wg, wb, gg, gb, ref, H, W, p, what):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    rg, rb, rdx, rdwg, rdwb = ref
    g, b = guidance_heads(x, wg, wb, H, W, guidance_dtype=F32)
    dx, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=F32)
    torch.cuda.synchronize()
    assert g.dtype == F32 and b.dtype == F32 and dx.dtype == x.dtype and dwg.dtype == F32 and dwb.dtype == F32
    e = {"guidance": _rel(g, rg), "blur": _rel(b, rb), "dwg": _rel(dwg, rdwg), "dwb": _rel(dwb, rdwb), "dx": _err16(dx, rdx, p)}
    print(what, {k: "%.2e" % v for k, v in e.items()})
    for k, v in e.items():
        assert v <= {"guidance": 1e-5, "blur": 1e-5, "dwg": 2e-5, "dwb": 2e-5, "dx": 1.0}[k], (what, k, v)
    return g, b, dx, dwg, dwb


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_forward_and_backward_against_the_float64_statement(dtn, shape):
    x, wg, wb, gg, gb, ref = _case(shape, dtn)
    _check(x, wg, wb, gg, gb, ref, shape[4], shape[5], DTS[dtn][1], "%s %s" % (dtn, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_a_view_of_x_one_element_into_its_buffer(dtn):
    """x 2-byte aligned only: the paired loads are misaligned; the results are those of the aligned tensor, bitwise"""
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    for shape in (SHAPES[1], SHAPES[2]):
        x, wg, wb, gg, gb, ref = _case(shape, dtn)
        H, W = shape[4], shape[5]
        xv = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")[1:].view_as(x).copy_(x)
        assert xv.data_ptr() % 4 == 2 and xv.is_contiguous()
        got = _check(xv, wg, wb, gg, gb, ref, H, W, DTS[dtn][1], "%s view %s" % (dtn, shape))
        want = guidance_heads(x, wg, wb, H, W, guidance_dtype=F32) + guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=F32)
        assert all(torch.equal(a, r) for a, r in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_without_a_blur_head(dtn):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    shape = SHAPES[1]
    x, wg, wb, gg, gb, _ = _case(shape, dtn)
    dt, p = DTS[dtn]
    H, W = shape[4], shape[5]
    rg, _, rdx, rdwg, _ = statement_grads(x.double(), wg.to(dt).double(), None, gg.to(dt).double(), None, H, W)
    g, b = guidance_heads(x, wg, None, H, W, guidance_dtype=F32)
    dx, dwg, dwb = guidance_heads_backward(x, wg, None, gg, None, guidance_dtype=F32)
    assert b is None and dwb is None and g.dtype == F32
    assert _rel(g, rg) <= 1e-5 and _rel(dwg, rdwg) <= 2e-5 and _err16(dx, rdx, p) <= 1.0
    assert torch.equal(g, guidance_heads(x, wg, wb, H, W, guidance_dtype=F32)[0])                  # the guidance planes do not depend on the blur head


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_nothing_is_rounded_on_the_way_out(dtn):
    """small integers times powers of two: every product and every partial sum is exact in float32, whatever the order, so the float32 guidance and blur equal
    the float64 statement bitwise -- and the float32 head on x.float().  The sums (multiples of 2^-8, up to 9 x 40 terms) exceed dt's precision: a rounding
    to dt would show."""
    from cspn_amd.train_utils import guidance_heads
    from test_head_kxk import statement
    dt = DTS[dtn][0]
    B, C, h, w, H, W = 2, 40, 3, 35, 5, 69
    gen = torch.Generator().manual_seed(5)
    x = (torch.randint(-32, 33, (B, C, h, w), generator=gen).float() / 32).cuda().to(dt)
    wg = (torch.randint(-7, 8, (8, C, 3, 3), generator=gen).float() / 8).cuda()
    wb = (torch.randint(-7, 8, (1, C, 3, 3), generator=gen).float() / 8).cuda()
    assert torch.equal(wg.to(dt).float(), wg) and torch.equal(x.float().to(dt), x)
    g, b = guidance_heads(x, wg, wb, H, W, guidance_dtype=F32)
    rg, rb = statement(x.double(), wg.double(), wb.double(), H, W)
    assert g.dtype == F32 and b.dtype == F32
    assert torch.equal(g.double(), rg) and torch.equal(b.double(), rb)
    assert not torch.equal(g.to(dt).float(), g)                                    # (the values do need more than dt holds)
    g32, b32 = guidance_heads(x.float(), wg, wb, H, W)
    assert torch.equal(g, g32) and torch.equal(b, b32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_backward_is_deterministic_and_subsets_return_none(dtn):
    from cspn_amd.train_utils import guidance_heads_backward
    x, wg, wb, gg, gb, _ = _case((2, 64, 5, 40, 9, 79), dtn)
    a = guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=F32)
    b = guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=F32)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    dx, n1, n2 = guidance_heads_backward(x, wg, wb, gg, gb, need_w=False, guidance_dtype=F32)
    assert n1 is None and n2 is None and torch.equal(dx, a[0])
    n0, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb, need_x=False, guidance_dtype=F32)
    assert n0 is None and torch.equal(dwg, a[1]) and torch.equal(dwb, a[2])
    assert all(t is None for t in guidance_heads_backward(x, wg, wb, gg, gb, need_x=False, need_w=False, guidance_dtype=F32))


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", sorted(DTS))
def test_module_train_step_is_the_manual_composition(dtn):
    """GuidanceHeads(64, 3)(x16) -> Affinity_Propagate(4, 3) with a sparse mask -> Wighted_L1_Loss -> backward(), against: the new forward, Affinity_Propagate,
    its backward, the new backward -- bitwise; float32 guidance reaches the ring with no cast in the graph"""
    import cspn_amd
    from cspn_amd.train_utils import Wighted_L1_Loss, guidance_heads, guidance_heads_backward
    dt = DTS[dtn][0]
    B, C, h, w = 2, 64, 6, 40
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, C, h, w, generator=gen, device="cuda").to(dt)
    sp = (torch.rand(B, 1, 2 * h, 2 * w, generator=gen, device="cuda") < 0.05).float() * 2.0
    label = torch.rand(B, 1, 2 * h, 2 * w, generator=gen, device="cuda") * 3 + 0.5
    torch.manual_seed(7)
    heads = cspn_amd.GuidanceHeads(C, 3).cuda()
    with torch.no_grad():
        heads.weight_blur.add_(0.05)
    prop, loss_fn = cspn_amd.Affinity_Propagate(4, 3), Wighted_L1_Loss()
    xa = x.clone().requires_grad_(True)
    g, b = heads(xa)
    assert g.dtype == F32 and b.dtype == F32 and g.grad_fn is b.grad_fn
    # the head's own node: nothing (no .float()) between it and the ring
    assert type(g.grad_fn).__name__ == "_GuidanceHeadsFunctionBackward" and g.grad_fn.path.fwd == "cspn_guidance_head_g16"
    out = prop(g, b, sp)
    loss = loss_fn(out, label)
    loss.backward()
    assert xa.grad.dtype == dt and heads.weight_guidance.grad.dtype == F32 and heads.weight_blur.grad.dtype == F32
    wg, wb = heads.weight_guidance.detach(), heads.weight_blur.detach()
    g0, b0 = guidance_heads(x, wg, wb, guidance_dtype=F32)
    assert torch.equal(g0, g) and torch.equal(b0, b)
    g1, b1 = g0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    out1 = prop(g1, b1, sp)
    loss_fn(out1, label).backward()
    assert torch.equal(out1, out) and g1.grad.dtype == F32
    dx, dwg, dwb = guidance_heads_backward(x, wg, wb, g1.grad, b1.grad, guidance_dtype=F32)
    assert torch.equal(xa.grad, dx) and torch.equal(heads.weight_guidance.grad, dwg) and torch.equal(heads.weight_blur.grad, dwb)
    assert float(dx.float().abs().max()) > 0 and float(dwg.abs().max()) > 0
    # weights that are dt themselves: the same call on .float() (exact), their gradients .to(dt)
    xc, wgc, wbc = x.clone().requires_grad_(True), wg.to(dt).requires_grad_(True), wb.to(dt).requires_grad_(True)
    g2, b2 = guidance_heads(xc, wgc, wbc, guidance_dtype=F32)
    assert torch.equal(g2, g) and torch.equal(b2, b)                               # (the engine rounds the masters to the same values)
    ((g2 * g1.grad).sum() + (b2 * b1.grad).sum()).backward()
    assert wgc.grad.dtype == dt and torch.equal(wgc.grad, dwg.to(dt)) and torch.equal(wbc.grad, dwb.to(dt)) and torch.equal(xc.grad, dx)


@pytest.mark.gpu
def test_the_other_paths_of_the_module_are_todays_functions():
    import cspn_amd
    from cspn_amd.train_utils import guidance_heads
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 33, 5, 37, generator=gen).cuda()
    for K in (3, 5):
        m = cspn_amd.GuidanceHeads(33, K, 9, 73).cuda()
        g, b = m(x)
        rg, rb = guidance_heads(x, m.weight_guidance, m.weight_blur, 9, 73)
        assert g.dtype == F32 and torch.equal(g, rg) and torch.equal(b, rb)
        assert type(g.grad_fn).__name__ == "_GuidanceHeadsFunctionBackward"
        assert g.grad_fn.path.fwd == ("cspn_guidance_head_f32" if K == 3 else "cspn_guidance_head_kxk_f32")
    for dt in (torch.float16, torch.bfloat16):
        m = cspn_amd.GuidanceHeads(33, 5, 9, 73).cuda()
        g, b = m(x.to(dt))
        rg, rb = guidance_heads(x.to(dt), m.weight_guidance, m.weight_blur, 9, 73)
        assert g.dtype == dt and b.dtype == F32 and torch.equal(g, rg) and torch.equal(b, rb)
        assert type(g.grad_fn).__name__ == "_GuidanceHeadsFunctionBackward" and g.grad_fn.path.fwd == "cspn_guidance_head_kxk_g16"


@pytest.mark.gpu
def test_return_codes():
    from cspn_amd import _lib
    fwd_n, fwd, bwd_n, bwd = (_lib.symbol(n) for n in NEW)
    BADARG, WORKSPACE = -1, -2
    F16, BF16 = _lib.DTYPES["float16"], _lib.DTYPES["bfloat16"]
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()   # noqa: E731
    x = torch.zeros(1, 4, 3, 3, device="cuda", dtype=torch.float16)
    w8, w1 = torch.zeros(8, 4, 3, 3, device="cuda"), torch.zeros(1, 4, 3, 3, device="cuda")
    g, b = torch.zeros(1, 8, 6, 6, device="cuda"), torch.zeros(1, 1, 6, 6, device="cuda")
    n = fwd_n(1, 4, 3, 3)
    assert n > 0 and fwd_n(1, 0, 3, 3) == 0
    ws = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    assert fwd(P(x), F16, P(w8), P(w1), P(g), P(b), 1, 4, 3, 3, 6, 6, P(ws), n, st) == 0
    assert fwd(P(x), BF16, P(w8), None, P(g), None, 1, 4, 3, 3, 6, 6, P(ws), n, st) == 0                  # no blur head
    assert fwd(P(x), F16, P(w8), P(w1), P(g), P(b), 0, 4, 3, 3, 6, 6, P(ws), n, st) == 0                  # an empty batch
    for bad in (0, 3):
        assert fwd(P(x), bad, P(w8), P(w1), P(g), P(b), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG         # dtype
    assert fwd(None, F16, P(w8), P(w1), P(g), P(b), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG
    assert fwd(P(x), F16, None, P(w1), P(g), P(b), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG
    assert fwd(P(x), F16, P(w8), P(w1), None, P(b), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG
    assert fwd(P(x) + 1, F16, P(w8), P(w1), P(g), P(b), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG         # not 2-byte aligned
    assert fwd(P(x), F16, P(w8), P(w1), P(g), None, 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG             # w_blur without blur_out
    assert fwd(P(x), F16, P(w8), P(w1), P(g), P(b), 1, 4, 3, 3, 7, 6, P(ws), n, st) == BADARG             # H > 2 h
    assert fwd(P(x), F16, P(w8), P(w1), P(g), P(b), 1, 4, 3, 3, 6, 6, P(ws), n - 1, st) == WORKSPACE      # too small
    assert fwd(P(x), F16, P(w8), P(w1), P(g), P(b), 1, 4, 3, 3, 6, 6, P(ws) + 8, n, st) == WORKSPACE      # misaligned
    dx, dwg, dwb = torch.empty_like(x), torch.empty_like(w8), torch.empty_like(w1)
    n = bwd_n(1, 4, 3, 3)
    assert n > 0 and bwd_n(0, 4, 3, 3) == 0
    ws = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    assert bwd(P(x), F16, P(w8), P(w1), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws), n, st) == 0
    for bad in (0, 3):
        assert bwd(P(x), bad, P(w8), P(w1), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG
    assert bwd(P(x), F16, P(w8), P(w1), None, P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG
    assert bwd(P(x), F16, P(w8), P(w1), P(g), P(b), P(dx) + 1, P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG   # grad_x not 2-byte aligned
    assert bwd(P(x), F16, P(w8), P(w1), P(g), None, P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG       # a blur head without its gradient
    assert bwd(P(x), F16, P(w8), None, P(g), None, P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws), n, st) == BADARG        # grad_w_blur without a blur head
    assert bwd(P(x), F16, P(w8), P(w1), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws), 64, st) == WORKSPACE
    assert bwd(P(x), F16, P(w8), P(w1), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, P(ws) + 8, n, st) == WORKSPACE
    assert bwd(P(x), F16, P(w8), P(w1), P(g), P(b), None, None, None, 1, 4, 3, 3, 6, 6, None, 0, st) == 0                  # nothing asked for
    torch.cuda.synchronize()
