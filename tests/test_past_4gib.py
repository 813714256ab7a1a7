"""GPU: every engine on a batch whose gate / guidance tensor is 4 GiB or larger -- are the addresses right past byte 2^32?

The pattern of every case: inputs made on the device from a seeded generator (random per element: a row fetched from another image cannot
pass); one call on the whole batch; the same call on contiguous sub-batches whose gates stay below 2 GiB (small offsets: the regime the
rest of the suite covers); whole batch against the sub-batch results over EVERY element, on the device; and three images -- image 0, the
image that holds byte 2^32 of the gate tensor, the last image -- against a float64 (or oracle) reference on the CPU, at the suite's own
tolerances.  Every batch has at least two images wholly past the line.

Whole batch against sub-batches is compared BITWISE for the per-step 2D kernels, the K x K engine, the 3D per-step kernels and the heads'
outputs and dL/dx: each output element is the result of one thread's fixed sequence of operations on that image's data; the batch size only
decides which workgroup computes it (the tile grid, the launch grid), never the order of a sum.  The two rings are NOT bitwise across batch
sizes: a row's slot in the ring follows its position in its workgroup's stream, which the plan cuts differently for another batch, and the
slot decides the order in which a pixel's eight products are added -- on an MI355X about 30 % of the pixels of a sub-batch differ from the
whole batch's, by at most 6.1e-5 where max|out| is 250 (2.4e-7 of it), both sides within 3e-7 (24 steps) of the oracle.  They, and all
gradients (the whole batch and its sub-batches may take different backward paths: checkpointed ring / per step, fused sweeps / per step),
are compared within the 4e-6 of max|ref| that tests/test_backward.py allows for another summation order; the heads' dL/dW is a sum over the
batch and is held to the float32 bound of tests/test_head_kxk.py.

A test skips only when the device has less free memory than the peak its docstring states (torch.cuda.max_memory_allocated of a run on an
MI355X, 288 GB)."""
import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd.functional import cspn3d_forward_absnorm
from helpers import assert_close, rel_err
from oracle import cspn2d_oracle, cspn3d_oracle, guidance_head_oracle
from oracle.backward import cspn2d_backward_oracle, cspn3d_backward_oracle
from test_backward import GFLOOR, GTOL
from test_gpu_parity import _forward, _plan_info
from test_head_kxk import statement, torch_kxk_norm
from test_head_kxk_g16 import _err16
from test_kernel_size import _torch_module, _torch_noneKxK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LINE = 1 << 32
H2, W2 = 304, 1216           # the KITTI image of the 2D cases
D3, H3, W3 = 16, 64, 256     # the 3D volume: 160 of them are 4.36 GB of gates (16 x 32 x 160 x 608 has the same layout at 10x the oracle's time)


# ---- the pattern ---------------------------------------------------------------------------------------------------------------------
def _need(gib):
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < gib * 2 ** 30:
        pytest.skip("%.1f GiB of device memory free, the test's peak is %.1f GiB" % (free / 2 ** 30, gib))
    torch.cuda.reset_peak_memory_stats(DEV)


def _done(what):
    torch.cuda.synchronize()
    print("%s: peak device memory %.1f GiB" % (what, torch.cuda.max_memory_allocated(DEV) / 2 ** 30))
    torch.cuda.empty_cache()


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _randn(gen, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=gen, device=DEV, dtype=dtype)


def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen, device=DEV)


def _sparse(gen, depth):
    """a mask of ~500 pinned pixels per KITTI image with depths of their own (config 4)"""
    m = (_rand(gen, *depth.shape) < 1.4e-3).float()
    return m * (_rand(gen, *depth.shape) * 80 + 0.1)


def _geometry(B, gate_bytes_per_image):
    """-> (the sub-batches [(a, b)] with gates below 2 GiB, the three anchored images); checks the conditions on the batch"""
    line = LINE // gate_bytes_per_image              # the image that holds byte 2^32 of the gate tensor
    assert B * gate_bytes_per_image >= LINE and line + 2 <= B - 1, "two images must lie wholly past the line"
    n = ((1 << 31) - 1) // gate_bytes_per_image
    subs = [(a, min(B, a + n)) for a in range(0, B, n)]
    assert all((b - a) * gate_bytes_per_image < 1 << 31 for a, b in subs) and len(subs) >= 3
    return subs, [0, line, B - 1]


def _cut(t, a, b):
    return None if t is None else t[a:b]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(whole, part, a, b, what):
    assert torch.equal(_bits(whole[a:b]), _bits(part)), "%s: images %d .. %d differ from the sub-batch call (%d elements)" % (
        what, a, b - 1, int((_bits(whole[a:b]) != _bits(part)).sum()))


def _near(whole, part, a, b, scale, what):
    w, p = whole[a:b].float(), part.float()
    assert torch.equal(torch.isfinite(w), torch.isfinite(p)), what
    err = float((w - p).abs().max()) / scale
    assert err <= 4e-6, "%s: images %d .. %d: %.3g of max|ref| from the sub-batch call" % (what, a, b - 1, err)


def _scale(t):
    return max(float(t.float().abs().max()), 1e-30)


def _cpu(t, i, f64=False):
    if t is None:
        return None
    c = t[i:i + 1].cpu()
    return c.double() if f64 else c.float()


def _grad_close(a, ref, what):
    assert_close(np.asarray(a, np.float64), np.asarray(ref, np.float64), what, rtol=GTOL, atol_frac=GFLOOR)


# ---- 2D, 3 x 3 ---------------------------------------------------------------------------------------------------------------------
B2 = 366                    # 366 x 304 x 1216: 135.3 M pixels, 4.33 GB of guidance; image 363 holds byte 2^32
FWD2D = [
    # id, W, n_iter, norm, mask, algo, what the dispatcher must say
    ("ring12x3", W2, 24, "8sum", True, "fused_ring12", None),            # the 12 x 3 ring, asked for by name (its table is too short for a linear plan: band groups)
    ("ring8x4-short-pass", W2, 12, "8sum", True, "auto", 8),             # a short first pass
    ("ring8x4-continuation", W2, 36, "8sum_abs", False, "auto", 8),      # a short first pass, then a continuation pass that reads its levels
    ("ring8x4-prenorm", W2, 24, "prenorm", True, "auto", 8),
    ("padded-rows", W2 - 2, 12, "8sum", False, "auto", "fused_padded"),  # W % 4 != 0: rows padded in the workspace
    ("per-step", W2, 3, "8sum_abs", True, "stepwise", None),             # one launch per iteration
    ("ring-compiled", W2, 24, "8sum", False, "fused_cxx", None),         # the compiler-generated ring (its image offset is an int, widened at the guidance)
]


@pytest.mark.parametrize("name,W,n_iter,norm,mask,algo,path", FWD2D, ids=[c[0] for c in FWD2D])
def test_2d_forward(name, W, n_iter, norm, mask, algo, path):
    """peak device memory 11.1 GiB (prenorm, which holds the raw guidance too: 15.1 GiB); 0.1 .. 0.9 s a case"""
    _need(15.1 if norm == "prenorm" else 11.1)
    B, H = B2, H2
    subs, anchors = _geometry(B, 32 * H * W)
    lib = cspn_amd.load()
    sub_algo = "fused_ring8" if path == 8 else algo   # (the sub-batches on the same ring, whatever the dispatcher prefers at their size)
    if path == 8:     # the dispatcher's own choice: the fused algo on the 8 x 4 ring
        assert lib.cspn2d_auto_algo(B, H, W, n_iter) == _lib.ALGOS["fused"]
        assert _lib.load_hooks().cspn_debug_fused2d_ring(B, H, W, int(mask)) == 8
        assert _plan_info(B, H, W)["stride"] > 2000   # one piece per CU of the linear plan: streams of more than 2000 rows
    elif path == "fused_padded":
        assert lib.cspn2d_auto_algo(B, H, W, n_iter) == _lib.ALGOS["fused_padded"]
    elif algo == "fused_ring12":   # asked for by name, the 12 x 3 ring runs every full first pass the assembly path takes
        assert _lib.load_hooks().cspn_debug_fused2d_ring(B, H, W, int(mask)) != 0
    gen = _gen(len(name) + n_iter)
    g = _randn(gen, B, 8, H, W)
    raw = g
    if norm == "prenorm":   # the engine reads the reference's gate_wb; the oracle below sees the raw guidance with '8sum'
        g = torch.cat([cspn_amd.cspn2d_normalize(raw[a:b], "8sum") for a, b in subs])
    h = _rand(gen, B, 1, H, W) * 80
    s = _sparse(gen, h) if mask else None
    out = _forward(g, h, s, n_iter, norm, algo)
    oracle = lambda i: cspn2d_oracle(_cpu(raw, i), _cpu(h, i), _cpu(s, i), n_iter, "8sum" if norm == "prenorm" else norm)
    differ, scale, exact = [], _scale(out), algo == "stepwise"   # (the per-step kernels: bitwise; the rings: see the module's docstring)
    for a, b in subs:
        part = _forward(g[a:b], h[a:b], _cut(s, a, b), n_iter, norm, sub_algo)
        n_bits = int((_bits(out[a:b]) != _bits(part)).sum())
        if n_bits and (exact or float((out[a:b] - part).abs().max()) > 4e-6 * scale):
            # the figures first: how far apart, and which of the two the oracle sides with (the first image that differs)
            i = a + int((_bits(out[a:b]) != _bits(part)).flatten(1).any(1).nonzero()[0])
            ref = oracle(i)
            differ.append((a, b - 1, n_bits, float((out[a:b] - part).abs().max()), i, rel_err(out[i:i + 1].cpu().numpy(), ref),
                           rel_err(part[i - a:i - a + 1].cpu().numpy(), ref)))
        del part
    print("%s: max|out| %.4g; sub-batches too far from the whole batch (first, last, elements, max |difference|, image, whole vs oracle, sub-batch vs "
          "oracle): %s" % (name, scale, differ))
    assert not differ, differ
    assert bool(torch.isfinite(out).all())
    if mask:
        assert torch.equal(out[s != 0], h[s != 0])   # pinned pixels are the blur depth exactly, in every image
    for i in anchors:
        assert_close(out[i:i + 1].cpu().numpy(), oracle(i), "%s, image %d" % (name, i))
    del g, raw, h, s, out
    _done(name)


def _backward_2d(B, n_iter, norm, name, expect_history):
    H, W = H2, W2
    assert (cspn_amd.cspn2d_history_bytes(B, H, W, n_iter) != 0) == expect_history
    gen = _gen(B + n_iter)
    g = _randn(gen, B, 8, H, W)
    h = _rand(gen, B, 1, H, W) * 80
    s = _sparse(gen, h)
    go = _randn(gen, B, 1, H, W)
    gg, gh = cspn_amd.cspn2d_backward(g, h, s, go, n_iter, norm)
    n = ((1 << 31) - 1) // (32 * H * W)
    sg, sh = _scale(gg), _scale(gh)
    for a in range(0, B, n):
        b = min(B, a + n)
        pg, ph = cspn_amd.cspn2d_backward(g[a:b], h[a:b], s[a:b], go[a:b], n_iter, norm)
        _near(gg, pg, a, b, sg, name + " dL/dguidance")
        _near(gh, ph, a, b, sh, name + " dL/dblur")
        del pg, ph
    return g, h, s, go, gg, gh


def test_2d_backward_past_the_line():
    """the per-step path (no history mode past the line), n_iter = 3: a workspace of 22 planes = 11.9 GB.  Peak device memory 21.2 GiB; 0.5 s"""
    _need(21.2)
    B, n_iter, norm = B2, 3, "8sum"
    subs, anchors = _geometry(B, 32 * H2 * W2)
    g, h, s, go, gg, gh = _backward_2d(B, n_iter, norm, "backward past the line", False)
    for i in anchors:
        _, rgg, rgh = cspn2d_backward_oracle(_cpu(g, i).numpy(), _cpu(h, i).numpy(), _cpu(s, i).numpy(), _cpu(go, i).numpy(), n_iter, norm)
        _grad_close(gg[i:i + 1].cpu().numpy(), rgg, "dL/dguidance, image %d" % i)
        _grad_close(gh[i:i + 1].cpu().numpy(), rgh, "dL/dblur, image %d" % i)
    del g, h, s, go, gg, gh
    _done("2D backward past the line")


def test_2d_backward_just_below_the_line():
    """the largest batch that keeps the checkpointed ring path (8 folded planes of B H W floats below 2^32 bytes: the per-lane offsets of
    the adjoint sweep reach the top of 32 bits), n_iter = 4.  Peak device memory 20.0 GiB; 0.5 s"""
    _need(20.0)
    B, n_iter, norm = 363, 4, "8sum_abs"
    assert 32 * B * H2 * W2 < LINE <= 32 * (B + 1) * H2 * W2
    g, h, s, go, gg, gh = _backward_2d(B, n_iter, norm, "backward below the line", True)
    for i in (0, B // 2, B - 1):
        _, rgg, rgh = cspn2d_backward_oracle(_cpu(g, i).numpy(), _cpu(h, i).numpy(), _cpu(s, i).numpy(), _cpu(go, i).numpy(), n_iter, norm)
        _grad_close(gg[i:i + 1].cpu().numpy(), rgg, "dL/dguidance, image %d" % i)
        _grad_close(gh[i:i + 1].cpu().numpy(), rgh, "dL/dblur, image %d" % i)
    del g, h, s, go, gg, gh
    _done("2D backward just below the line")


# ---- 2D, K x K ---------------------------------------------------------------------------------------------------------------------
def _kxk_gates(gen, N, K, H, W, dtype=torch.float32):
    """signed gates whose abs-sum stays near 1 (tests/test_kernel_size.py _gates)"""
    return (_randn(gen, N, K * K - 1, H, W) * (1.2 / (K * K - 1))).to(dtype)


HK, WK = 128, 512   # the K x K image: the kernels choose their path by W % 4 and alignment alone, and 8 x 8 tiles are a grid of many blocks
KXK = [
    # id, K, N, W, contract
    ("none-7", 7, 344, WK, "none"),          # 344 x 128 x 512: 4.33 GB of gates, image 341 holds byte 2^32
    ("none-7-odd-width", 7, 345, WK - 1, "none"),   # W % 4 != 0: the guarded scalar kernels (image 342 holds the byte)
    ("none-5", 5, 685, WK, "none"),          # 685 images of 24 planes: 4.31 GB, image 682 holds the byte
    ("norm-7", 7, 344, WK, "norm"),          # Affinity_Propagate over 7 x 7 (cspn2d_*_kxk_norm), '8sum', a mask
    ("absnorm-7", 7, 344, WK, "absnorm"),    # the demo module's step inside the engine (absnorm_propagate)
]


@pytest.mark.parametrize("name,K,N,W,contract", KXK, ids=[c[0] for c in KXK])
def test_kxk_forward_and_backward(name, K, N, W, contract):
    """n_iter = 2.  Peak device memory 14.8 GiB (norm-7: 17.0 GiB); 0.2 .. 1.3 s a case"""
    _need(17.0 if contract == "norm" else 14.8)
    H, n = HK, 2
    P = K * K - 1
    subs, anchors = _geometry(N, 4 * P * H * W)
    gen = _gen(K + N + W)
    g = _kxk_gates(gen, N, K, H, W) if contract != "norm" else _randn(gen, N, P, H, W)
    x = _rand(gen, N, 1, H, W) * 4 - 1
    s = _sparse(gen, x) if contract == "norm" else None
    go = _randn(gen, N, 1, H, W)
    if contract == "none":
        fwd = lambda g_, x_, s_: cspn_amd.cspn2d_forward_kxk(g_, x_, K, n)
        bwd = lambda g_, x_, s_, go_: cspn_amd.cspn2d_backward_kxk(g_, x_, go_, K, n)
        ref = lambda g_, x_, s_: _torch_noneKxK(g_, x_, K, n)
    elif contract == "norm":
        fwd = lambda g_, x_, s_: cspn_amd.cspn2d_forward_kxk_norm(g_, x_, s_, K, n, "8sum")
        bwd = lambda g_, x_, s_, go_: cspn_amd.cspn2d_backward_kxk_norm(g_, x_, s_, go_, K, n, "8sum")
        ref = lambda g_, x_, s_: torch_kxk_norm(g_, x_, s_, K, n, "8sum")
    else:
        fwd = lambda g_, x_, s_: cspn_amd.cspn2d_forward_kxk_absnorm(g_, x_, K, n)
        bwd = lambda g_, x_, s_, go_: cspn_amd.cspn2d_backward_kxk_absnorm(g_, x_, go_, K, n)
        ref = lambda g_, x_, s_: _torch_module(g_, x_, K, n)
    out = fwd(g, x, s)
    gg, gx = bwd(g, x, s, go)
    sg, sx = _scale(gg), _scale(gx)
    for a, b in subs:
        _same(out, fwd(g[a:b], x[a:b], _cut(s, a, b)), a, b, name)
        pg, px = bwd(g[a:b], x[a:b], _cut(s, a, b), go[a:b])
        _near(gg, pg, a, b, sg, name + " gate gradient")
        _near(gx, px, a, b, sx, name + " value gradient")
        del pg, px
    for i in anchors:
        gr, xr = _cpu(g, i, True).requires_grad_(True), _cpu(x, i, True).requires_grad_(True)
        r = ref(gr, xr, _cpu(s, i, True))
        r.backward(_cpu(go, i, True))
        assert_close(out[i:i + 1].cpu().numpy(), r.detach().numpy(), "%s, image %d" % (name, i))
        _grad_close(gg[i:i + 1].cpu().numpy(), gr.grad.numpy(), "%s gate gradient, image %d" % (name, i))
        _grad_close(gx[i:i + 1].cpu().numpy(), xr.grad.numpy(), "%s value gradient, image %d" % (name, i))
    del g, x, s, go, out, gg, gx
    _done(name)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_kxk_16_bit_gates_past_2_to_the_30_elements(dtype):
    """16-bit gates cannot reach 4 GiB before the element limit refuses them; their element index passes 2^30 (a 2 x index in 32 bits would
    wrap).  344 x 48 x 128 x 512 = 1.082e9 gates.  Forward: bitwise the float32 engine on gate.float() of the sub-batches (the property of
    tests/test_kxk_g16.py); gate gradient: the float32 engine's, rounded once.  Peak device memory 9.9 GiB; 0.2 .. 1.3 s"""
    _need(9.9)
    K, N, H, W, n = 7, 344, HK, WK, 2
    P = K * K - 1
    assert 1 << 30 <= N * P * H * W <= 0x7fffffff
    n_sub = ((1 << 31) - 1) // (4 * P * H * W)      # sub-batches whose float32 gates stay below 2 GiB
    gen = _gen(16)
    g = _kxk_gates(gen, N, K, H, W, dtype)
    x = _rand(gen, N, 1, H, W) * 4 - 1
    go = _randn(gen, N, 1, H, W)
    out = cspn_amd.cspn2d_forward_kxk(g, x, K, n)
    gg, gx = cspn_amd.cspn2d_backward_kxk(g, x, go, K, n)
    assert out.dtype == torch.float32 and gg.dtype == dtype and gx.dtype == torch.float32
    for a in range(0, N, n_sub):
        b = min(N, a + n_sub)
        wide = g[a:b].float()
        _same(out, cspn_amd.cspn2d_forward_kxk(wide, x[a:b], K, n), a, b, "forward")
        pg, px = cspn_amd.cspn2d_backward_kxk(wide, x[a:b], go[a:b], K, n)
        _same(gx, px, a, b, "value gradient")
        _same(gg, pg.to(dtype), a, b, "gate gradient")
        del wide, pg, px
    for i in (0, (1 << 30) // (P * H * W), N - 1):     # the middle one holds gate number 2^30
        gr, xr = _cpu(g, i, True).requires_grad_(True), _cpu(x, i, True).requires_grad_(True)
        r = _torch_noneKxK(gr, xr, K, n)
        r.backward(_cpu(go, i, True))
        assert_close(out[i:i + 1].cpu().numpy(), r.detach().numpy(), "image %d" % i)
        _grad_close(gx[i:i + 1].cpu().numpy(), xr.grad.numpy(), "value gradient, image %d" % i)
        eps = 2.0 ** (-11 if dtype == torch.float16 else -8)   # the float32 bound and one rounding to the gate's type
        assert_close(gg[i:i + 1].float().cpu().numpy(), gr.grad.numpy(), "gate gradient, image %d" % i, rtol=GTOL + eps, atol_frac=GFLOOR)
    del g, x, go, out, gg, gx
    _done("K x K, %s gates" % dtype)


# ---- 3D ----------------------------------------------------------------------------------------------------------------------------
B3 = 160     # 160 x 16 x 64 x 256: 41.9 M voxels, 4.36 GB of gates; volume 157 holds byte 2^32, volumes 158 and 159 lie past it


def _gates3(gen, dtype=torch.float32):
    g = _rand(gen, B3, 26, D3, H3, W3)
    g /= g.sum(1, keepdim=True) + 0.3       # the Paddle contract: gates used as given, their sum below 1
    return g.to(dtype)


def test_3d_stepwise_forward_and_the_persistent_kernel_declines():
    """algo 'stepwise' (n_iter = 2) in the normalising mode (27 folded planes: a 4.7 GB workspace) and on the Paddle contract; the
    persistent kernel indexes the gates with 32-bit byte offsets and declines every batch of 4 GiB of gates or more
    (persistent3d_supported): asked for by name it is an error, 'auto' runs the per-step kernels.  Peak device memory 8.9 GiB; 0.4 s"""
    _need(8.9)
    subs, anchors = _geometry(B3, 4 * 26 * D3 * H3 * W3)
    # the largest batch whose gates stay below 2^32 bytes is taken, one volume more is not: what declines is 4 * 26 * B * V < 2^32
    below = LINE // (4 * 26 * D3 * H3 * W3)
    assert 4 * 26 * below * D3 * H3 * W3 < LINE <= 4 * 26 * (below + 1) * D3 * H3 * W3
    assert cspn_amd.load().cspn3d_multi_supported(below, 1, D3, H3, W3, 12) == 1
    assert cspn_amd.load().cspn3d_multi_supported(below + 1, 1, D3, H3, W3, 12) == 0
    assert not cspn_amd.load().cspn3d_multi_supported(B3, 1, D3, H3, W3, 12)
    gen = _gen(3)
    g = _gates3(gen)
    h = _rand(gen, B3, 1, D3, H3, W3)
    with pytest.raises(_lib.CspnError, match="persistent 3D kernel does not take this call"):
        cspn_amd.cspn3d_forward(g, h, None, 12, "none", "persistent")
    cspn_amd.cspn3d_check_status()
    for norm, algo, n in (("8sum_abs", "stepwise", 2), ("none", "stepwise", 2), ("none", "auto", 12)):
        out = cspn_amd.cspn3d_forward(g, h, None, n, norm, algo)
        for a, b in subs:
            _same(out, cspn_amd.cspn3d_forward(g[a:b], h[a:b], None, n, norm, "stepwise"), a, b, "3D %s %s" % (norm, algo))
        for i in anchors:
            assert_close(out[i:i + 1].cpu().numpy(), cspn3d_oracle(_cpu(g, i), _cpu(h, i), None, n, norm), "3D %s %s, volume %d" % (norm, algo, i))
        del out
    cspn_amd.cspn3d_check_status()
    del g, h
    _done("3D forward")


def test_3d_backward():
    """cspn3d_backward, n_iter = 2.  Peak device memory 14.6 GiB; 0.7 s"""
    _need(14.6)
    subs, anchors = _geometry(B3, 4 * 26 * D3 * H3 * W3)
    gen, n = _gen(4), 2
    g = _gates3(gen)
    h = _rand(gen, B3, 1, D3, H3, W3)
    go = _randn(gen, B3, 1, D3, H3, W3)
    gg, gf = cspn_amd.cspn3d_backward(g, h, go, n)
    sg, sf = _scale(gg), _scale(gf)
    for a, b in subs:
        pg, pf = cspn_amd.cspn3d_backward(g[a:b], h[a:b], go[a:b], n)
        _near(gg, pg, a, b, sg, "3D gate gradient")
        _near(gf, pf, a, b, sf, "3D value gradient")
        del pg, pf
    for i in anchors:
        rg, rf = cspn3d_backward_oracle(_cpu(g, i).numpy(), _cpu(h, i).numpy(), _cpu(go, i).numpy(), n, dtype=np.float64)
        _grad_close(gg[i:i + 1].cpu().numpy(), rg, "3D gate gradient, volume %d" % i)
        _grad_close(gf[i:i + 1].cpu().numpy(), rf, "3D value gradient, volume %d" % i)
    cspn_amd.cspn3d_check_status()
    del g, h, go, gg, gf
    _done("3D backward")


def test_3d_absnorm_forward_float32_and_16_bit():
    """cspn3d_forward_absnorm (the demo's module: raw guide, normalised into the workspace, then the per-step kernels), float32 and bfloat16 guides (the 16-bit guide stays below
    4 GiB; its element index passes 2^30).  Peak device memory 10.8 GiB; 0.5 s"""
    _need(10.8)
    subs, anchors = _geometry(B3, 4 * 26 * D3 * H3 * W3)
    gen, n = _gen(5), 2
    guide = _randn(gen, B3, 26, D3, H3, W3)
    h = _rand(gen, B3, 1, D3, H3, W3)
    assert 1 << 30 <= guide.numel() <= 0x7fffffff
    for dtype in (torch.float32, torch.bfloat16):
        gd = guide.to(dtype)
        out = cspn3d_forward_absnorm(gd, h, n, "stepwise")
        for a, b in subs:
            _same(out, cspn3d_forward_absnorm(gd[a:b].float(), h[a:b], n, "stepwise"), a, b, "3D absnorm %s" % dtype)
        for i in anchors:
            w = _cpu(gd, i, True).abs()
            w = (w / w.sum(1, keepdim=True)).float()
            assert_close(out[i:i + 1].cpu().numpy(), cspn3d_oracle(w, _cpu(h, i), None, n, "none"), "3D absnorm %s, volume %d" % (dtype, i))
        del gd, out
    cspn_amd.cspn3d_check_status()
    del guide, h
    _done("3D absnorm")


# ---- the guidance heads ------------------------------------------------------------------------------------------------------------
def test_head_kxk_7_forward_and_gradients():
    """guidance_heads for K = 7 at 64 x 304 x 1216 from x [64, 64, 152, 608]: 4.54 GB of guidance; image 60 holds byte 2^32.  Forward and
    dL/dx bitwise the sub-batch calls, dL/dW the sum over the sub-batches within the float32 bound of tests/test_head_kxk.py.
    Peak device memory 14.3 GiB; 6.5 s (the float64 statement of three images)"""
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    _need(14.3)
    B, C, h, w, P = 64, 64, H2 // 2, W2 // 2, 48
    subs, anchors = _geometry(B, 4 * P * H2 * W2)
    gen = _gen(7)
    x = _randn(gen, B, C, h, w)
    wg = _randn(gen, P, C, 3, 3) / (3.0 * C ** 0.5)
    wb = _randn(gen, 1, C, 3, 3) / (3.0 * C ** 0.5)
    g, b_ = guidance_heads(x, wg, wb, H2, W2)
    gg = _randn(gen, B, P, H2, W2)
    gb = _randn(gen, B, 1, H2, W2)
    dx, dwg, dwb = guidance_heads_backward(x, wg, wb, gg, gb)
    swg, swb = torch.zeros_like(dwg, dtype=torch.float64), torch.zeros_like(dwb, dtype=torch.float64)
    for a, b in subs:
        pg, pb = guidance_heads(x[a:b], wg, wb, H2, W2)
        _same(g, pg, a, b, "K = 7 head, guidance")
        _same(b_, pb, a, b, "K = 7 head, blur")
        pdx, pdwg, pdwb = guidance_heads_backward(x[a:b], wg, wb, gg[a:b], gb[a:b])
        _same(dx, pdx, a, b, "K = 7 head, dL/dx")
        swg += pdwg.double()
        swb += pdwb.double()
        del pg, pb, pdx
    assert float((dwg.double() - swg).abs().max()) <= 2e-5 * float(swg.abs().max())
    assert float((dwb.double() - swb).abs().max()) <= 2e-5 * float(swb.abs().max())
    for i in anchors:
        xr = _cpu(x, i, True).requires_grad_(True)     # (the float64 statement; dL/dW is not anchored, so only x asks for a gradient)
        rg, rb = statement(xr, wg.double().cpu(), wb.double().cpu(), H2, W2)
        rdx, = torch.autograd.grad((rg * _cpu(gg, i, True)).sum() + (rb * _cpu(gb, i, True)).sum(), xr)
        rg, rb = rg.detach(), rb.detach()
        for got, ref, what in ((g, rg, "guidance"), (b_, rb, "blur"), (dx, rdx, "dL/dx")):
            err = float((got[i:i + 1].cpu().double() - ref).abs().max() / ref.abs().max())
            assert err <= 1e-5, ("K = 7 head", what, i, err)
    del x, g, b_, gg, gb, dx
    _done("K = 7 head")


def test_head_kxk_7_bfloat16():
    """the 16-bit K = 7 head: x and the guidance in bfloat16 (2.27 GB of guidance, element index past 2^30).  Peak device memory 4.4 GiB; 3.7 s"""
    from cspn_amd.train_utils import guidance_heads
    _need(4.4)
    B, C, h, w, P, dt = 64, 64, H2 // 2, W2 // 2, 48, torch.bfloat16
    assert 1 << 30 <= B * P * H2 * W2
    n_sub = ((1 << 31) - 1) // (4 * P * H2 * W2)
    gen = _gen(8)
    x = _randn(gen, B, C, h, w).to(dt)
    wg = _randn(gen, P, C, 3, 3) / (3.0 * C ** 0.5)
    wb = _randn(gen, 1, C, 3, 3) / (3.0 * C ** 0.5)
    g, b_ = guidance_heads(x, wg, wb, H2, W2)
    assert g.dtype == dt and b_.dtype == torch.float32
    for a in range(0, B, n_sub):
        b = min(B, a + n_sub)
        pg, pb = guidance_heads(x[a:b], wg, wb, H2, W2)
        _same(g, pg, a, b, "bfloat16 head, guidance")
        _same(b_, pb, a, b, "bfloat16 head, blur")
        del pg, pb
    for i in (0, (1 << 30) // (P * H2 * W2), B - 1):
        rg, rb = statement(_cpu(x, i, True), wg.to(dt).double().cpu(), wb.to(dt).double().cpu(), H2, W2)
        assert _err16(g[i:i + 1].cpu(), rg, 8) <= 1.0
        assert float((b_[i:i + 1].cpu().double() - rb).abs().max() / rb.abs().max()) <= 1e-5
    del x, g, b_
    _done("bfloat16 K = 7 head")


def test_head_3x3_past_2_to_the_27_pixels():
    """the 8-plane head at 366 x 304 x 1216 (4.33 GB of guidance) from x [366, 16, 152, 608].
    Peak device memory 9.3 GiB; 1.7 s"""
    from cspn_amd.train_utils import guidance_heads
    _need(9.3)
    B, C, h, w = B2, 16, H2 // 2, W2 // 2
    subs, anchors = _geometry(B, 32 * H2 * W2)
    gen = _gen(9)
    x = _randn(gen, B, C, h, w)
    wg = _randn(gen, 8, C, 3, 3) / (3.0 * C ** 0.5)
    wb = _randn(gen, 1, C, 3, 3) / (3.0 * C ** 0.5)
    g, b_ = guidance_heads(x, wg, wb, H2, W2)
    for a, b in subs:
        pg, pb = guidance_heads(x[a:b], wg, wb, H2, W2)
        _same(g, pg, a, b, "3 x 3 head, guidance")
        _same(b_, pb, a, b, "3 x 3 head, blur")
        del pg, pb
    for i in anchors:
        rg, rb = guidance_head_oracle(_cpu(x, i).numpy(), wg.cpu().numpy(), wb.cpu().numpy(), H2, W2)
        assert float(np.abs(g[i:i + 1].cpu().numpy() - rg).max() / np.abs(rg).max()) <= 1e-5
        assert float(np.abs(b_[i:i + 1].cpu().numpy() - rb).max() / np.abs(rb).max()) <= 1e-5
    del x, g, b_
    _done("3 x 3 head")
