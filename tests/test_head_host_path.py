"""The one host path of the four guidance-head paths in train_utils (float32 8-plane, float32 24 / 48 planes, 16-bit 24 / 48 planes with 16-bit guidance, 16-bit
8-plane with float32 guidance): guidance_heads, guidance_heads_backward and the one autograd Function against the C ABI itself, called here through
_lib.symbol with a workspace of the test's own -- bit for bit (torch.equal): the host path adds no arithmetic, and every backward is deterministic
(test_backward_is_deterministic_* in the heads' own test files)."""
import inspect

import pytest
import torch

F32 = torch.float32
PLANES_TO_K = {8: 3, 24: 5, 48: 7}
# the ABI of each path, written out: forward, its workspace query, backward, its workspace query
ABI = {"A": ("cspn_guidance_head_f32", "cspn_guidance_head_workspace_bytes", "cspn_guidance_head_backward_f32", "cspn_guidance_head_backward_workspace_bytes"),
       "B": ("cspn_guidance_head_kxk_f32", "cspn_guidance_head_kxk_workspace_bytes", "cspn_guidance_head_kxk_backward_f32",
             "cspn_guidance_head_kxk_backward_workspace_bytes"),
       "C": ("cspn_guidance_head_kxk_g16", "cspn_guidance_head_kxk_g16_workspace_bytes", "cspn_guidance_head_kxk_backward_g16",
             "cspn_guidance_head_kxk_backward_g16_workspace_bytes"),
       "D": ("cspn_guidance_head_g16", "cspn_guidance_head_g16_workspace_bytes", "cspn_guidance_head_backward_g16", "cspn_guidance_head_backward_g16_workspace_bytes")}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_the_table_is_complete_and_nothing_is_left_behind():
    from cspn_amd import _lib, train_utils
    names = {n for p in train_utils._HEAD_PATHS.values() for n in (p.fwd, p.fwd_ws, p.bwd, p.bwd_ws)}
    assert names == {n for row in ABI.values() for n in row} and names <= set(_lib._SYMBOLS)
    source = inspect.getsource(train_utils)
    for gone in ("late_symbol", "_lib.load(", "current_stream"):
        assert gone not in source, gone
    functions = [c for c in vars(train_utils).values() if isinstance(c, type) and issubclass(c, torch.autograd.Function) and "Heads" in c.__name__]
    assert len(functions) == 1, functions


# ---------------------------------------------------------------------------------------------------------------- GPU
SHAPES = [(2, 20, 3, 5, 5, 9),           # C no multiple of 16, narrowed output, odd W
          (1, 4, 1, 1, 2, 2)]            # one pixel, C below one matrix step
# id -> (path, guidance planes, dtype of x, guidance_dtype argument)
CASES = {"A": ("A", 8, F32, None), "B24": ("B", 24, F32, None), "B48": ("B", 48, F32, None),
         "C-float16": ("C", 24, torch.float16, None), "C-bfloat16": ("C", 24, torch.bfloat16, None),
         "D-float16": ("D", 8, torch.float16, F32), "D-bfloat16": ("D", 8, torch.bfloat16, F32)}
_CACHE = {}


def _inputs(case, shape):
    """-> x, the float32 master weights, dL/dguidance in the path's guidance dtype, dL/dblur float32, on the GPU; made once, never written to"""
    if (case, shape) not in _CACHE:
        path, P, dt, _ = CASES[case]
        B, C, h, w, H, W = shape
        gen = torch.Generator().manual_seed(100 * P + C + (dt == torch.bfloat16))
        x = torch.randn(B, C, h, w, generator=gen).cuda().to(dt)
        wg, wb = (torch.randn(P, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)).cuda(), (torch.randn(1, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)).cuda()
        gg = torch.randn(B, P, H, W, generator=gen).cuda().to(dt if path == "C" else F32)
        gb = torch.randn(B, 1, H, W, generator=gen).cuda()
        _CACHE[case, shape] = (x, wg, wb, gg, gb)
    return _CACHE[case, shape]


def _abi_call(path, backward, x, wg, tensors, H, W, norm="none"):
    """the C ABI as include/cspn_amd.h declares it: x [, dtype], the tensors, B, C, h, w, H, W [, K | norm_type], workspace, its bytes, stream"""
    from cspn_amd import _lib
    B, C, h, w = x.shape
    K = PLANES_TO_K[int(wg.shape[0])]
    name, query = ABI[path][2:] if backward else ABI[path][:2]
    n = _lib.symbol(query)(*{"A": (B, C, h, w) if backward else (C,), "B": (B, C, h, w, K), "C": (B, C, h, w, K), "D": (B, C, h, w)}[path])
    ws = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    code = (_lib.DTYPES[str(x.dtype).split(".")[1]],) if path in "CD" else ()
    tail = {"A": () if backward else (_lib.NORM_TYPES[norm],), "B": (K,), "C": (K,), "D": ()}[path]
    rc = _lib.symbol(name)(x.data_ptr(), *code, wg.data_ptr(), *(t.data_ptr() if t is not None else None for t in tensors), B, C, h, w, H, W, *tail,
                           ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)


def abi_forward(path, x, wg, wb, H, W, norm="none"):
    B, P = x.shape[0], wg.shape[0]
    g = torch.empty(B, P, H, W, dtype=x.dtype if path == "C" else F32, device="cuda")
    b = torch.empty(B, 1, H, W, device="cuda") if wb is not None else None
    _abi_call(path, False, x, wg, (wb, g, b), H, W, norm)
    return g, b


def abi_backward(path, x, wg, wb, gg, gb):
    dx, dwg, dwb = torch.empty_like(x), torch.empty_like(wg), torch.empty_like(wb) if wb is not None else None
    _abi_call(path, True, x, wg, (wb, gg, gb, dx, dwg, dwb), gg.shape[2], gg.shape[3])
    return dx, dwg, dwb


def _same(got, want):
    assert len(got) == len(want)
    for a, r in zip(got, want):
        assert (a is None and r is None) or (a.dtype == r.dtype and torch.equal(a, r))


def _autograd_step(x, wg, wb, gg, gb, H, W, gd):
    """.grad of x and the weights after one step on (guidance * gg).sum() + (blur * gb).sum(); gg or gb None: that output stays out of the loss"""
    from cspn_amd.train_utils import guidance_heads
    xa, wga, wba = (t.clone().requires_grad_(True) if t is not None else None for t in (x, wg, wb))
    g, b = guidance_heads(xa, wga, wba, H, W, guidance_dtype=gd)
    assert g.grad_fn is not None and (b is None or b.grad_fn is g.grad_fn)
    sum((o * r).sum() for o, r in ((g, gg), (b, gb)) if r is not None).backward()
    return g.detach(), xa.grad, wga.grad, wba.grad if wba is not None else None


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [True, False], ids=["blur", "noblur"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", sorted(CASES))
def test_each_path_is_the_raw_abi_call(case, shape, blur):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    path, _, _, gd = CASES[case]
    x, wg, wb, gg, gb = _inputs(case, shape)
    if not blur:
        wb = gb = None
    H, W = shape[4:]
    want = abi_forward(path, x, wg, wb, H, W)
    _same(guidance_heads(x, wg, wb, H, W, guidance_dtype=gd), want)
    want_grads = abi_backward(path, x, wg, wb, gg, gb)
    _same(guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=gd), want_grads)
    g, *grads = _autograd_step(x, wg, wb, gg, gb, H, W, gd)
    _same([g] + grads, [want[0]] + list(want_grads))
    if path == "A":   # the normalisation fused behind the conv, with grad off
        with torch.no_grad():
            _same(guidance_heads(x, wg, wb, H, W, "8sum"), abi_forward(path, x, wg, wb, H, W, "8sum"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in sorted(CASES) if c[0] in "CD"])
def test_weights_of_xs_dtype_are_widened_exactly_and_their_gradients_come_back_in_it(case):
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    path, _, dt, gd = CASES[case]
    shape = SHAPES[0]
    x, wg, wb, gg, gb = _inputs(case, shape)
    H, W = shape[4:]
    wg, wb = wg.to(dt), wb.to(dt)
    want = abi_forward(path, x, wg.float(), wb.float(), H, W)
    dx, dwg, dwb = abi_backward(path, x, wg.float(), wb.float(), gg, gb)
    want_grads = (dx, dwg.to(dt), dwb.to(dt))
    _same(guidance_heads(x, wg, wb, H, W, guidance_dtype=gd), want)
    _same(guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=gd), want_grads)
    g, *grads = _autograd_step(x, wg, wb, gg, gb, H, W, gd)
    _same([g] + grads, [want[0]] + list(want_grads))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in sorted(CASES) if c != "B48"])
def test_a_missing_output_gradient_is_zeros_of_the_paths_gradient_dtype(case):
    from cspn_amd.train_utils import guidance_heads_backward
    gd = CASES[case][3]
    shape = SHAPES[0]
    x, wg, wb, gg, gb = _inputs(case, shape)
    H, W = shape[4:]
    _, *grads = _autograd_step(x, wg, wb, None, gb, H, W, gd)                      # the loss uses blur only
    _same(grads, guidance_heads_backward(x, wg, wb, torch.zeros_like(gg), gb, guidance_dtype=gd))
    _, *grads = _autograd_step(x, wg, wb, gg, None, H, W, gd)                      # the loss uses guidance only
    _same(grads, guidance_heads_backward(x, wg, wb, gg, torch.zeros_like(gb), guidance_dtype=gd))
