"""The guidance heads for 5x5 and 7x7 propagation: Simple_Gudi_UpConv_Block_Last_Layer(C, K*K-1, ...) (reference
cspn_pytorch/models/torch_resnet_cspn_nyu.py:187-206: Unpool :41-54 + bias-free 3x3 conv; the class takes the plane count as an argument) with the 1-plane blur
head riding along -- cspn_guidance_head_kxk_f32 / cspn_guidance_head_kxk_backward_f32, train_utils.guidance_heads with weight_guidance [24 | 48, C, 3, 3].
Golden vectors: tests/golden/head_kxk_golden.npz, outputs and autograd gradients of the UNMODIFIED reference class (tests/golden/make_head_kxk_golden.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "head_kxk_golden.npz"))
NAMES = sorted({k.split("/")[0] for k in GOLD.files})
PLANES = {5: 24, 7: 48}


def _case(name):
    g = {k.split("/")[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}
    return g, int(g["meta"][0]), int(g["meta"][1]), int(g["meta"][2])


def _rel(a, b):
    """max |a - b| over max |b| (the plane maximum of tests/test_head.py)"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert bool(torch.isfinite(a).all())
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


# ---- the float64 torch statement of the head: conv_transpose2d Unpool, narrow, conv2d ----
def statement(x, wg, wb, oh=0, ow=0):
    """-> (guidance [B,P,H,W], blur [B,1,H,W] | None) in the dtype of x (the tests call it in float64); differentiable"""
    C = x.shape[1]
    up = torch.zeros(C, 1, 2, 2, dtype=x.dtype, device=x.device)
    up[:, :, 0, 0] = 1
    U = TF.conv_transpose2d(x, up, stride=2, groups=C)
    if oh and ow:
        U = U[:, :, :oh, :ow]
    return TF.conv2d(U, wg, padding=1), (TF.conv2d(U, wb, padding=1) if wb is not None else None)


def statement_grads(x, wg, wb, gg, gb, oh=0, ow=0):
    xs, wgs = x.double().clone().requires_grad_(True), wg.double().clone().requires_grad_(True)
    wbs = wb.double().clone().requires_grad_(True) if wb is not None else None
    g, b = statement(xs, wgs, wbs, oh, ow)
    loss = (g * gg.double()).sum()
    if wb is not None:
        loss = loss + (b * gb.double()).sum()
    loss.backward()
    return g.detach(), (b.detach() if b is not None else None), xs.grad, wgs.grad, (wbs.grad if wbs is not None else None)


# ---- the float64 torch statement of the K x K contract (as tests/test_kxk_norm.py torch_kxk_norm: cspn.py:42-144 with the ZeroPad2d tuples generalised) ----
def torch_kxk_norm(guidance, blur, sparse, K, n, norm):
    R = K // 2
    P = [(l, K - 1 - l, t, K - 1 - t) for t in range(K) for l in range(K) if (t, l) != (R, R)]
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([TF.pad(g[:, k], P[k]) for k in range(len(P))], 1)
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, R:-R, R:-R]
    gate = gate.unsqueeze(2)
    m = sparse.sign() if sparse is not None else None
    x = blur
    for _ in range(n):
        xp = torch.stack([TF.pad(x, P[k]) for k in range(len(P))], 1)
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, R:-R, R:-R]
        if m is not None:
            x = (1 - m) * x + m * blur
    return x


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", NAMES)
def test_statement_vs_reference_golden(name):
    """the float64 statement reproduces what the unmodified reference class returned, and what autograd computed through it"""
    c, oh, ow, K = _case(name)
    t = {k: torch.from_numpy(v) for k, v in c.items() if k != "meta"}
    assert t["wg"].shape[0] == PLANES[K] == K * K - 1
    g, b, dx, dwg, dwb = statement_grads(t["x"], t["wg"], t["wb"], t["grad_guidance"], t["grad_blur"], oh, ow)
    assert _rel(g, t["guidance"]) <= 2e-6 and _rel(b, t["blur"]) <= 2e-6
    assert _rel(dx, t["grad_x"]) <= 1e-5 and _rel(dwg, t["grad_wg"]) <= 1e-5 and _rel(dwb, t["grad_wb"]) <= 1e-5


def test_golden_covers_both_kernels_and_the_shapes():
    ks = {int(GOLD[n + "/meta"][2]) for n in NAMES}
    assert ks == {5, 7} and len(NAMES) == 12
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "head_kxk_golden.npz")) < 1 << 20


def test_statement_at_24_planes_is_three_8_plane_statements():
    gen = torch.Generator().manual_seed(24)
    x = torch.randn(2, 6, 5, 7, generator=gen, dtype=torch.float64)
    wg = torch.randn(24, 6, 3, 3, generator=gen, dtype=torch.float64)
    wb = torch.randn(1, 6, 3, 3, generator=gen, dtype=torch.float64)
    g, b = statement(x, wg, wb, 9, 13)
    parts = [statement(x, wg[s:s + 8], wb, 9, 13) for s in (0, 8, 16)]
    assert g.shape == (2, 24, 9, 13) and torch.allclose(g, torch.cat([p[0] for p in parts], 1), rtol=0, atol=1e-12)
    assert all(torch.equal(p[1], b) for p in parts)


def test_new_symbols_are_declared_and_exported():
    import cspn_amd
    from cspn_amd import _lib
    names = ["cspn_guidance_head_kxk_workspace_bytes", "cspn_guidance_head_kxk_f32", "cspn_guidance_head_kxk_backward_workspace_bytes",
             "cspn_guidance_head_kxk_backward_f32"]
    header = open(os.path.join(ROOT, "include", "cspn_amd.h")).read()
    for n in names:
        assert n in _lib._LATE_SYMBOLS and (n + "(") in header
    assert "#define CSPN_ABI_VERSION 5" in header
    assert {"guidance_heads", "guidance_heads_backward"} <= set(cspn_amd.__all__)


def test_python_argument_errors_without_gpu():
    """the checks that come before any tensor reaches the engine"""
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    x = torch.zeros(1, 4, 3, 3)
    with pytest.raises(ValueError, match="8 \\| 24 \\| 48"):
        guidance_heads(x, torch.zeros(16, 4, 3, 3))
    with pytest.raises(ValueError, match="8 \\| 24 \\| 48"):
        guidance_heads_backward(x, torch.zeros(16, 4, 3, 3), None, torch.zeros(1, 16, 6, 6), None)
    with pytest.raises(ValueError, match="\\[B,C,h,w\\]"):
        guidance_heads(x[0], torch.zeros(24, 4, 3, 3))
    with pytest.raises(ValueError, match="\\[B,C,h,w\\]"):
        guidance_heads_backward(x[0], torch.zeros(24, 4, 3, 3), None, torch.zeros(1, 24, 6, 6), None)
    with pytest.raises(ValueError, match="same device"):
        guidance_heads(x, torch.zeros(24, 4, 3, 3, device="meta"))
    with pytest.raises(ValueError, match="same device"):
        guidance_heads_backward(x, torch.zeros(24, 4, 3, 3), None, torch.zeros(1, 24, 6, 6, device="meta"), None)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(B, C, h, w, H, W, K, seed, scale=None):
    gen = torch.Generator().manual_seed(seed)
    P = PLANES[K]
    s = scale if scale is not None else 3.0 * C ** 0.5
    x = torch.randn(B, C, h, w, generator=gen)
    wg = torch.randn(P, C, 3, 3, generator=gen) / s
    wb = torch.randn(1, C, 3, 3, generator=gen) / s
    gg, gb = torch.randn(B, P, H, W, generator=gen), torch.randn(B, 1, H, W, generator=gen)
    return [t.cuda() for t in (x, wg, wb, gg, gb)]


def _check_all(x, wg, wb, gg, gb, oh, ow, what):
    """engine forward + the three gradients against the float64 statement on the same device: outputs and dL/dx <= 1e-5, dL/dW <= 2e-5"""
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    rg, rb, rdx, rdwg, rdwb = statement_grads(x, wg, wb, gg, gb, oh, ow)
    g, b = guidance_heads(x, wg, wb, oh, ow)
    dx, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb)
    torch.cuda.synchronize()
    errs = {"guidance": _rel(g, rg), "dx": _rel(dx, rdx), "dwg": _rel(dwg, rdwg)}
    if wb is not None:
        errs["blur"], errs["dwb"] = _rel(b, rb), _rel(dwb, rdwb)
    else:
        assert b is None and dwb is None
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= (2e-5 if k in ("dwg", "dwb") else 1e-5), (what, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_engine_vs_reference_golden(name):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    c, oh, ow, K = _case(name)
    t = {k: _dev(v) for k, v in c.items() if k != "meta"}
    g, b = guidance_heads(t["x"], t["wg"], t["wb"], oh, ow)
    dx, dwg, dwb = guidance_heads_backward(t["x"], t["wg"], t["wb"], t["grad_guidance"], t["grad_blur"])
    torch.cuda.synchronize()
    errs = [_rel(g, c["guidance"]), _rel(b, c["blur"]), _rel(dx, c["grad_x"]), _rel(dwg, c["grad_wg"]), _rel(dwb, c["grad_wb"])]
    print(name, ["%.2e" % e for e in errs])
    assert g.shape == c["guidance"].shape and b.shape == c["blur"].shape
    assert errs[0] <= 1e-5 and errs[1] <= 1e-5 and errs[2] <= 1e-5 and errs[3] <= 2e-5 and errs[4] <= 2e-5
    g2, none = guidance_heads(t["x"], t["wg"], None, oh, ow)                      # guidance only
    assert none is None and torch.equal(g2, g)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("B,h,w,oh,ow", [(2, 114, 152, 228, 304), (1, 152, 608, 304, 1216), (3, 40, 125, 79, 249)])
def test_engine_vs_fp64_statement_at_the_reference_sizes(K, B, h, w, oh, ow):
    _check_all(*_inputs(B, 64, h, w, oh, ow, K, B + h + w + K), oh, ow, "K%d B%d %dx%d -> %dx%d" % (K, B, h, w, oh, ow))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_engine_fuzzed_small_odd_shapes(K):
    """seeded small shapes: 1 .. 3 images, C in {1, 5, 33, 64}, heights 1 .. 9, widths below, at and above the kernels' 32-column tiles and 8-pixel tiles;
    exact 2x and narrowed outputs incl. odd sizes; with and without the blur head"""
    rng = np.random.default_rng(500 + K)
    for case in range(24):
        B, C = int(rng.integers(1, 4)), int(rng.choice([1, 5, 33, 64]))
        h = int(rng.integers(1, 10))
        w = int(rng.choice([1, 2, 3, 7, 9, 31, 32, 33, 65]))
        oh, ow = 0, 0
        if rng.random() < 0.6:
            oh, ow = int(rng.integers(max(1, 2 * h - 3), 2 * h + 1)), int(rng.integers(max(1, 2 * w - 3), 2 * w + 1))
        H, W = (oh, ow) if oh else (2 * h, 2 * w)
        x, wg, wb, gg, gb = _inputs(B, C, h, w, H, W, K, 1000 * K + case, scale=3.0)
        if case % 4 == 3:
            wb, gb = None, None
        _check_all(x, wg, wb, gg, gb, oh, ow, "K%d case %d: B%d C%d h%d w%d -> %dx%d" % (K, case, B, C, h, w, H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_engine_vs_concatenated_8_plane_heads(K):
    """24 / 48 planes against torch.cat of today's 8-plane head on weight slices (not bitwise: the summation order differs)"""
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    B, C, h, w, oh, ow = 2, 64, 21, 70, 41, 139
    x, wg, wb, gg, gb = _inputs(B, C, h, w, oh, ow, K, 77 + K)
    g, b = guidance_heads(x, wg, wb, oh, ow)
    dx, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb)
    parts = [guidance_heads(x, wg[s:s + 8].contiguous(), wb, oh, ow) for s in range(0, PLANES[K], 8)]
    assert _rel(g, torch.cat([p[0] for p in parts], 1)) <= 1e-5 and _rel(b, parts[0][1]) <= 1e-5
    rdx, rdwg, rdwb = torch.zeros_like(x), [], None
    for i, s in enumerate(range(0, PLANES[K], 8)):
        first = i == 0          # the blur head's gradient rides with the first slice only
        pdx, pdwg, pdwb = guidance_heads_backward(x, wg[s:s + 8].contiguous(), wb if first else None, gg[:, s:s + 8].contiguous(), gb if first else None)
        rdx += pdx
        rdwg.append(pdwg)
        rdwb = pdwb if first else rdwb
    assert _rel(dx, rdx) <= 1e-5 and _rel(dwg, torch.cat(rdwg, 0)) <= 2e-5 and _rel(dwb, rdwb) <= 2e-5


@pytest.mark.gpu
def test_k3_through_the_new_entry_points_is_the_8_plane_head():
    import cspn_amd
    from cspn_amd import _lib
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    lib = cspn_amd.load()
    B, C, h, w, H, W = 2, 20, 9, 70, 17, 139
    gen = torch.Generator().manual_seed(3)
    x, wg, wb = (torch.randn(*s, generator=gen).cuda() for s in ((B, C, h, w), (8, C, 3, 3), (1, C, 3, 3)))
    gg, gb = torch.randn(B, 8, H, W, generator=gen).cuda(), torch.randn(B, 1, H, W, generator=gen).cuda()
    rg, rb = guidance_heads(x, wg, wb, H, W)
    rdx, rdwg, rdwb = guidance_heads_backward(x, wg, wb, gg, gb)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()   # noqa: E731
    n = _lib.late_symbol("cspn_guidance_head_kxk_workspace_bytes")(B, C, h, w, 3)
    assert n == lib.cspn_guidance_head_workspace_bytes(C)
    ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
    g, b = torch.empty_like(rg), torch.empty_like(rb)
    assert _lib.late_symbol("cspn_guidance_head_kxk_f32")(P(x), P(wg), P(wb), P(g), P(b), B, C, h, w, H, W, 3, P(ws), n, st) == 0
    n = _lib.late_symbol("cspn_guidance_head_kxk_backward_workspace_bytes")(B, C, h, w, 3)
    assert n == lib.cspn_guidance_head_backward_workspace_bytes(B, C, h, w)
    ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dx, dwg, dwb = torch.empty_like(x), torch.empty_like(wg), torch.empty_like(wb)
    assert _lib.late_symbol("cspn_guidance_head_kxk_backward_f32")(P(x), P(wg), P(wb), P(gg), P(gb), P(dx), P(dwg), P(dwb), B, C, h, w, H, W, 3, P(ws), n, st) == 0
    torch.cuda.synchronize()
    for a, r in ((g, rg), (b, rb), (dx, rdx), (dwg, rdwg), (dwb, rdwb)):
        assert torch.equal(a, r)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_backward_is_deterministic_and_subsets_return_none(K):
    from cspn_amd.train_utils import guidance_heads_backward
    x, wg, wb, gg, gb = _inputs(2, 64, 37, 150, 73, 299, K, 9 + K)
    a = guidance_heads_backward(x, wg, wb, gg, gb)
    b = guidance_heads_backward(x, wg, wb, gg, gb)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    dx, n1, n2 = guidance_heads_backward(x, wg, wb, gg, gb, need_w=False)
    assert n1 is None and n2 is None and torch.equal(dx, a[0])
    n0, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb, need_x=False)
    assert n0 is None and torch.equal(dwg, a[1]) and torch.equal(dwb, a[2])
    dx2, dwg2, none = guidance_heads_backward(x, wg, None, gg, None)                # guidance head only
    r = statement_grads(x, wg, None, gg, None, 73, 299)
    assert none is None and _rel(dx2, r[2]) <= 1e-5 and _rel(dwg2, r[3]) <= 2e-5
    assert all(t is None for t in guidance_heads_backward(x, wg, wb, gg, gb, need_x=False, need_w=False))


@pytest.mark.gpu
def test_autograd_function_and_frozen_weights():
    from cspn_amd.train_utils import guidance_heads
    x, wg, wb, gg, gb = _inputs(2, 33, 9, 70, 17, 139, 5, 31)
    rg, rb, rdx, rdwg, rdwb = statement_grads(x, wg, wb, gg, gb, 17, 139)
    xa, wga, wba = (t.clone().requires_grad_(True) for t in (x, wg, wb))
    g, b = guidance_heads(xa, wga, wba, 17, 139)
    assert g.grad_fn is not None and g.grad_fn is b.grad_fn                       # one autograd Function for both heads
    ((g * gg).sum() + (b * gb).sum()).backward()
    assert _rel(xa.grad, rdx) <= 1e-5 and _rel(wga.grad, rdwg) <= 2e-5 and _rel(wba.grad, rdwb) <= 2e-5
    xc = x.clone().requires_grad_(True)                                             # frozen weights: only dL/dx is computed
    g, b = guidance_heads(xc, wg, wb, 17, 139)
    ((g * gg).sum() + (b * gb).sum()).backward()
    assert torch.equal(xc.grad, xa.grad)


@pytest.mark.gpu
def test_heads_plus_kxk_propagation_train_step_vs_torch_fp64():
    """guidance_heads (24 planes) -> Affinity_PropagateKxK(n, 5, '8sum') with a sparse mask -> loss.backward(): output <= 1e-5, dL/dx and both weight gradients
    <= 2e-4 against torch autograd in float64 through the statement of the head and the statement of the contract"""
    import cspn_amd
    from cspn_amd.train_utils import guidance_heads
    B, C, h, w, N, K = 2, 16, 20, 70, 12, 5
    gen = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(B, C, h, w, generator=gen, device="cuda")
    wg = torch.randn(24, C, 3, 3, generator=gen, device="cuda") / 12
    wb = torch.randn(1, C, 3, 3, generator=gen, device="cuda") / 12 + 0.05
    sp = (torch.rand(B, 1, 2 * h, 2 * w, generator=gen, device="cuda") < 0.03).float() * 2.0
    go = torch.randn(B, 1, 2 * h, 2 * w, generator=gen, device="cuda")
    xa, wga, wba = (t.clone().requires_grad_(True) for t in (x, wg, wb))
    g, b = guidance_heads(xa, wga, wba)
    out = cspn_amd.Affinity_PropagateKxK(N, K, "8sum")(g, b, sp)
    (out * go).sum().backward()
    xb, wgb, wbb = (t.double().clone().requires_grad_(True) for t in (x, wg, wb))
    rg, rb = statement(xb, wgb, wbb)
    ref = torch_kxk_norm(rg, rb, sp.double(), K, N, "8sum")
    (ref * go.double()).sum().backward()
    eo = _rel(out.detach(), ref.detach())
    eg = {n: _rel(a, r) for a, r, n in ((xa.grad, xb.grad, "x"), (wga.grad, wgb.grad, "wg"), (wba.grad, wbb.grad, "wb"))}
    print("train step: out %.2e" % eo, {k: "%.2e" % v for k, v in eg.items()})
    assert eo <= 1e-5
    for n, v in eg.items():
        assert v <= 2e-4, (n, v)


@pytest.mark.gpu
def test_argument_errors_and_return_codes():
    from cspn_amd import _lib
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    x = torch.zeros(1, 4, 3, 3, device="cuda")
    w24, w5 = torch.zeros(24, 4, 3, 3, device="cuda"), torch.zeros(1, 4, 3, 3, device="cuda")
    with pytest.raises(ValueError, match="8 \\| 24 \\| 48"):
        guidance_heads(x, torch.zeros(16, 4, 3, 3, device="cuda"))
    with pytest.raises(ValueError, match="Affinity_PropagateKxK"):
        guidance_heads(x, w24, w5, norm_type="8sum")
    with pytest.raises(ValueError, match="same device"):
        guidance_heads(x, w24.cpu(), w5)
    with pytest.raises(ValueError, match="same device"):
        guidance_heads_backward(x, w24, w5, torch.zeros(1, 24, 6, 6), torch.zeros(1, 1, 6, 6, device="cuda"))
    fwd_n, fwd = _lib.late_symbol("cspn_guidance_head_kxk_workspace_bytes"), _lib.late_symbol("cspn_guidance_head_kxk_f32")
    bwd_n, bwd = _lib.late_symbol("cspn_guidance_head_kxk_backward_workspace_bytes"), _lib.late_symbol("cspn_guidance_head_kxk_backward_f32")
    BADARG, WORKSPACE = -1, -2
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()   # noqa: E731
    g, b = torch.zeros(1, 24, 6, 6, device="cuda"), torch.zeros(1, 1, 6, 6, device="cuda")
    n = fwd_n(1, 4, 3, 3, 5)
    assert n > 0 and fwd_n(1, 4, 3, 3, 4) == 0
    ws = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    assert fwd(P(x), P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == 0
    assert fwd(P(x), P(w24), None, P(g), None, 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == 0                 # no blur head
    assert fwd(P(x), P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 4, P(ws), n, st) == BADARG           # K
    assert fwd(P(x), P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 7, 6, 5, P(ws), n, st) == BADARG           # H > 2 h
    assert fwd(P(x), P(w24), P(w5), P(g), None, 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG           # w_blur without blur_out
    assert fwd(P(x), P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws), n - 1, st) == WORKSPACE    # too small
    assert fwd(P(x), P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 5, P(ws) + 8, n, st) == WORKSPACE    # misaligned
    assert fwd(P(x), P(w24), P(w5), P(g), P(b), 1, 4, 3, 3, 6, 6, 3, P(ws), 8, st) == WORKSPACE        # K = 3: the same code, not the 8-plane head's -1
    dx, dwg, dwb = torch.empty_like(x), torch.empty_like(w24), torch.empty_like(w5)
    n = bwd_n(1, 4, 3, 3, 5)
    assert n > 0 and bwd_n(0, 4, 3, 3, 5) == 0 and bwd_n(1, 4, 3, 3, 9) == 0
    ws = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    assert bwd(P(x), P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == 0
    assert bwd(P(x), P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 6, P(ws), n, st) == BADARG
    assert bwd(P(x), P(w24), P(w5), P(g), None, P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG      # a blur head without its gradient
    assert bwd(P(x), P(w24), None, P(g), None, P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), n, st) == BADARG       # grad_w_blur without a blur head
    assert bwd(P(x), P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 7, 5, P(ws), n, st) == BADARG      # W > 2 w
    assert bwd(P(x), P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws), 64, st) == WORKSPACE
    assert bwd(P(x), P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 1, 4, 3, 3, 6, 6, 5, P(ws) + 8, n, st) == WORKSPACE
    assert bwd(P(x), P(w24), P(w5), P(g), P(b), None, None, None, 1, 4, 3, 3, 6, 6, 5, None, 0, st) == 0                 # nothing asked for: nothing needed
    assert bwd(P(x), P(w24), P(w5), P(g), P(b), P(dx), P(dwg), P(dwb), 0, 4, 3, 3, 6, 6, 5, None, 0, st) == 0            # empty batch
    torch.cuda.synchronize()
