"""fp16 / bf16 gates and guidance in the 2D K x K engine (cspn2d_*_kxk*_g16), forward and backward.

The contract is exact widening: a 16-bit gate is widened to float32 where it is used and all arithmetic is the float32 engine's in its
order, so the forward and grad_x / grad_blur are bitwise the float32 engine's on gate.float(), and the gradient with respect to the 16-bit
tensor is bitwise fp32_engine_grad.to(dtype) (accumulated in float32, rounded once).  No tolerance appears below except
RTOL = 1e-4 against the float64 torch statements, the bound the float32 engine's own tests use
(the conv weights' gradients behind the module are compared bitwise too, see test_module_under_autocast_reaches_the_conv)."""
import ctypes
import os
import re

import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F
from test_kernel_size import RTOL, _rel, _torch_noneKxK
from test_kxk_norm import torch_kxk_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_forward_kxk_g16", "cspn2d_backward_kxk_g16", "cspn2d_forward_kxk_norm_g16", "cspn2d_backward_kxk_norm_g16"]
DTYPES = [torch.float16, torch.bfloat16]
F16, BF16 = 1, 2


# ---- CPU ----
def test_new_symbols_are_exported_declared_and_the_abi_stays_5():
    raw = open(os.path.join(ROOT, "include", "cspn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert re.search(r"CSPN_DTYPE_F16\s*=\s*1\b", text) and re.search(r"CSPN_DTYPE_BF16\s*=\s*2\b", text)
    assert _lib.DTYPES == {"float16": F16, "bfloat16": BF16}
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert re.search(r"#define\s+CSPN_ABI_VERSION\s+5\b", raw)


def test_abi_argument_errors_of_the_none_op_without_gpu():
    lib = cspn_amd.load()
    fwd = _lib.late_symbol("cspn2d_forward_kxk_g16")
    bwd = _lib.late_symbol("cspn2d_backward_kxk_g16")
    g, x, o, h, w, gg, gx = (ctypes.c_void_p(i << 32) for i in range(1, 8))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 20
    odd = lambda p: ctypes.c_void_p(p.value + 1)   # noqa: E731
    # forward: (gate, gate_dtype, x, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
    for dt in (F16, BF16):
        for dtype in (0, 3, -1, 16):
            assert fwd(g, dtype, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"dtype" in err()
        assert fwd(odd(g), dt, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"2-byte aligned" in err()
        for K in (3, 4, 9, 0):
            assert fwd(g, dt, x, o, None, 0, 2, 1, 8, 8, K, 3, w, M, None) == -1 and b"K must be" in err()
        assert fwd(None, dt, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"null" in err()
        assert fwd(g, dt, None, o, None, 0, 2, 1, 8, 8, 5, 3, w, M, None) == -1
        assert fwd(g, dt, x, None, None, 0, 2, 1, 8, 8, 5, 3, w, M, None) == -1
        for B, C, H, W in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (-1, 1, 8, 8)):
            assert fwd(g, dt, x, o, None, 0, B, C, H, W, 5, 3, w, M, None) == -1 and b"bad shape" in err()
        assert fwd(g, dt, x, o, None, 0, 2, 1, 8, 8, 5, -1, w, M, None) == -1
        assert fwd(g, dt, x, x, None, 0, 2, 1, 8, 8, 7, 3, w, M, None) == -1 and b"alias" in err()
        assert fwd(g, dt, x, g, None, 0, 2, 1, 8, 8, 7, 3, w, M, None) == -1 and b"alias" in err()
        assert fwd(g, dt, x, ctypes.c_void_p((1 << 32) + 64), None, 0, 2, 1, 8, 8, 5, 3, w, M, None) == -1   # out inside the gates
        # the 16-bit gates end after 2 * 24 * 128 = 6144 bytes: an out right behind them is no alias (the float32 gates would reach it)
        assert fwd(g, dt, x, ctypes.c_void_p(g.value + 6144), None, 0, 2, 1, 8, 8, 5, 3, None, 0, None) == -2
        assert fwd(g, dt, x, ctypes.c_void_p(g.value + 6140), None, 0, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"alias" in err()
        assert fwd(g, dt, x, o, x, M, 2, 1, 8, 8, 5, 3, None, 0, None) == -1 and b"alias" in err()   # history on the input
        assert fwd(g, dt, x, o, None, 0, 2, 1, 8, 8, 5, 3, None, 0, None) == -2 and b"workspace" in err()
        assert fwd(g, dt, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, 100, None) == -2
        assert fwd(g, dt, x, o, None, 0, 2, 1, 8, 8, 5, 3, ctypes.c_void_p((6 << 32) + 4), M, None) == -2 and b"aligned" in err()
        assert fwd(g, dt, x, o, h, 100, 2, 1, 8, 8, 5, 3, None, 0, None) == -2 and b"history" in err()
        assert fwd(g, dt, x, o, None, 0, 1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3, w, M, None) == -3   # 2^32 elements
        assert fwd(g, dt, x, o, None, 0, 1 << 8, 1, 1 << 10, 1 << 8, 7, 3, w, M, None) == -3       # 48 2^26 gate elements
        # backward: (gate, gate_dtype, x, history, history_bytes, grad_out, grad_gate, grad_x, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
        hbytes = 4 * 2 * 8 * 8 * 2
        assert bwd(g, 7, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"dtype" in err()
        assert bwd(odd(g), dt, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"2-byte aligned" in err()
        assert bwd(g, dt, x, h, hbytes, o, odd(gg), gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"2-byte aligned" in err()
        assert bwd(g, dt, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 9, 3, w, M, None) == -1 and b"K must be" in err()
        assert bwd(None, dt, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"null" in err()
        assert bwd(g, dt, None, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1
        assert bwd(g, dt, x, h, hbytes, None, gg, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1
        assert bwd(g, dt, x, h, hbytes, o, gg, gx, 0, 1, 8, 8, 5, 3, w, M, None) == -1 and b"bad shape" in err()
        assert bwd(g, dt, x, None, 0, o, gg, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"history" in err()
        assert bwd(g, dt, x, h, 64, o, gg, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"history" in err()
        assert bwd(g, dt, x, h, hbytes, o, gg, gg, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, h, hbytes, o, gg, o, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, h, hbytes, o, x, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, h, hbytes, o, g, gx, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, h, hbytes, o, gg, h, 2, 1, 8, 8, 5, 3, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, None, 0, None) == -2 and b"workspace" in err()
        assert bwd(g, dt, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, 64, None) == -2
        assert bwd(g, dt, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, ctypes.c_void_p((6 << 32) + 4), M, None) == -2 and b"aligned" in err()
        assert bwd(g, dt, x, h, hbytes, o, gg, gx, 1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3, w, M, None) == -3
        assert bwd(g, dt, x, None, 0, o, None, None, 2, 1, 8, 8, 5, 3, w, M, None) == 0   # nothing asked for: checked, nothing launched


def test_abi_argument_errors_of_the_norm_contract_without_gpu():
    lib = cspn_amd.load()
    fwd = _lib.late_symbol("cspn2d_forward_kxk_norm_g16")
    bwd = _lib.late_symbol("cspn2d_backward_kxk_norm_g16")
    g, x, s, o, h, w, gg, gx = (ctypes.c_void_p(i << 32) for i in range(1, 9))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    odd = lambda p: ctypes.c_void_p(p.value + 1)   # noqa: E731
    # forward: (guidance, gate_dtype, blur, sparse, out, history, history_bytes, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream)
    for dt in (F16, BF16):
        for dtype in (0, 3, -2):
            assert fwd(g, dtype, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"dtype" in err()
        assert fwd(odd(g), dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"2-byte aligned" in err()
        for K in (1, 2, 4, 9, 0):
            assert fwd(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, K, 3, 0, w, M, None) == -1 and b"K must be" in err()
        for norm in (2, 3, -1, 7):
            assert fwd(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, norm, w, M, None) == -1 and b"norm" in err()
        for sc, sp in ((2, s), (4, s), (0, s), (1, None), (3, None), (-1, s)):
            assert fwd(g, dt, x, sp, o, None, 0, 2, 3, sc, 8, 8, 5, 3, 0, w, M, None) == -1 and b"sparse_C" in err()
        assert fwd(None, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"null" in err()
        assert fwd(g, dt, None, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1
        assert fwd(g, dt, x, None, None, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1
        for B, C, H, W in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -2)):
            assert fwd(g, dt, x, None, o, None, 0, B, C, 0, H, W, 5, 3, 0, w, M, None) == -1 and b"bad shape" in err()
        assert fwd(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, -1, 0, w, M, None) == -1
        assert fwd(g, dt, x, s, x, None, 0, 2, 1, 1, 8, 8, 7, 3, 1, w, M, None) == -1 and b"alias" in err()
        assert fwd(g, dt, x, s, s, None, 0, 2, 1, 1, 8, 8, 3, 3, 1, w, M, None) == -1 and b"alias" in err()   # out on the mask
        assert fwd(g, dt, x, None, ctypes.c_void_p((1 << 32) + 64), None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1   # out inside the guidance
        assert fwd(g, dt, x, None, o, x, M, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()   # history on the input
        assert fwd(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, ctypes.c_void_p(g.value + 256), M, None) == -1 and b"alias" in err()
        assert fwd(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, None, 0, None) == -2 and b"workspace" in err()
        assert fwd(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, 100, None) == -2
        assert fwd(g, dt, x, None, o, h, M, 2, 1, 0, 8, 8, 5, 3, 0, w, 100, None) == -2   # with a history the fold still needs room
        assert fwd(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, ctypes.c_void_p((6 << 32) + 4), M, None) == -2 and b"aligned" in err()
        assert fwd(g, dt, x, None, o, h, 100, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -2 and b"history" in err()
        assert fwd(g, dt, x, None, o, None, 0, 1 << 12, 1 << 8, 0, 1 << 6, 1 << 6, 5, 3, 0, w, M, None) == -3   # 2^32 elements
        assert fwd(g, dt, x, None, o, None, 0, 1 << 8, 1, 0, 1 << 10, 1 << 8, 7, 3, 0, w, M, None) == -3       # 48 2^26 guidance elements
        assert fwd(g, dt, x, s, o, None, 0, 1 << 8, 4, 4, 1 << 10, 1 << 8, 3, 3, 0, w, M, None) == -3        # per-channel w': 2^31 elements
        # backward: (guidance, gate_dtype, blur, sparse, history, history_bytes, grad_out, grad_guidance, grad_blur, B, C, sparse_C, H, W, K,
        #            n_iter, norm, ws, ws_bytes, stream)
        hbytes = 4 * 2 * 8 * 8 * 2
        assert bwd(g, 0, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"dtype" in err()
        assert bwd(odd(g), dt, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"2-byte aligned" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, odd(gg), gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"2-byte aligned" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 9, 3, 0, w, M, None) == -1 and b"K must be" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 2, w, M, None) == -1 and b"norm" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, gx, 2, 2, 2, 8, 8, 5, 3, 0, w, M, None) == -1 and b"sparse_C" in err()
        assert bwd(None, dt, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"null" in err()
        assert bwd(g, dt, x, None, h, hbytes, None, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1
        assert bwd(g, dt, x, None, None, 0, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"history" in err()
        assert bwd(g, dt, x, None, h, 64, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"history" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, gg, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, o, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, x, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, s, h, hbytes, o, gg, s, 2, 1, 1, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, h, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, None, 0, None) == -2 and b"workspace" in err()
        assert bwd(g, dt, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, 64, None) == -2
        assert bwd(g, dt, x, None, h, hbytes, o, gg, gx, 1 << 12, 1 << 8, 0, 1 << 6, 1 << 6, 5, 3, 0, w, M, None) == -3


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_argument_errors_without_gpu(dtype):
    g5, x = torch.rand(1, 24, 6, 9).to(dtype), torch.rand(1, 2, 6, 9).to(dtype)
    with pytest.raises(ValueError, match="gate must be"):
        F.cspn2d_forward_kxk(g5, x, 7, 3)
    with pytest.raises(ValueError, match="gate must be"):
        F.cspn2d_forward_kxk(g5[:, :23], x, 5, 3)
    with pytest.raises(ValueError, match="x has shape"):
        F.cspn2d_forward_kxk(g5, x[:, :, :5], 5, 3)
    with pytest.raises(ValueError, match="kernel_size"):
        F.cspn2d_forward_kxk(g5, x, 4, 3)
    with pytest.raises(ValueError, match="n_iter"):
        F.cspn2d_forward_kxk(g5, x, 5, -1)
    with pytest.raises(ValueError, match="grad_out"):
        F.cspn2d_backward_kxk(g5, x, x[:, :1], 5, 3)
    with pytest.raises(ValueError, match="gate_weight must have"):
        cspn_amd.affinity_propagate(x, g5, 7, 2)
    s = torch.rand(1, 1, 6, 9).to(dtype)
    with pytest.raises(ValueError, match="guidance must be"):
        F.cspn2d_forward_kxk_norm(g5, x, s, 7, 3)
    with pytest.raises(ValueError, match="blur_depth has shape"):
        F.cspn2d_forward_kxk_norm(g5, x[:, :, :, :8], s, 5, 3)
    with pytest.raises(ValueError, match="sparse_depth"):
        F.cspn2d_forward_kxk_norm(g5, x, s[:, :, :5], 5, 3)
    with pytest.raises(ValueError, match="norm_type"):
        F.cspn2d_forward_kxk_norm(g5, x, s, 5, 3, "none")
    with pytest.raises(ValueError, match="grad_out"):
        F.cspn2d_backward_kxk_norm(g5, x, s, x[:, :1], 5, 3)
    # n_iter == 0: the input object itself, whatever its dtype
    assert F.cspn2d_forward_kxk(g5, x, 5, 0) is x
    assert F.cspn2d_forward_kxk_norm(g5, x, s, 5, 0) is x
    assert cspn_amd.affinity_propagate(x, g5, 5, 0) is x
    assert cspn_amd.Affinity_PropagateKxK(0, 5)(g5, x, s) is x
    assert cspn_amd.Affinity_Propagate(0, 3)(g5[:, :8], x, s) is x
    # the engine has no CPU path for any dtype
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn2d_forward_kxk(g5, x, 5, 3)


@pytest.mark.gpu
def test_float64_and_the_normaliser_still_raise_typeerror_on_the_device():
    """(on a CPU tensor the engine reports the device first, so the dtype errors can only be seen with device tensors)"""
    g5, x = torch.rand(1, 24, 6, 9, device="cuda"), torch.rand(1, 2, 6, 9, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        F.cspn2d_forward_kxk(g5.double(), x, 5, 3)
    with pytest.raises(TypeError, match="float32"):
        F.cspn2d_forward_kxk(g5.half(), x.double(), 5, 3)
    with pytest.raises(TypeError, match="float32"):
        F.cspn2d_backward_kxk(g5.half(), x, x.double(), 5, 3)
    with pytest.raises(TypeError, match="float32"):
        F.cspn2d_forward_kxk_norm(g5.double(), x, None, 5, 3)
    with pytest.raises(TypeError, match="float32"):
        F.cspn2d_forward_kxk_norm(g5.bfloat16(), x.double(), None, 5, 3)
    with pytest.raises(TypeError, match="float32"):
        cspn_amd.affinity_propagate(x.double(), g5.half(), 5, 2)
    for dtype in DTYPES:
        with pytest.raises(TypeError, match="float32"):
            cspn_amd.gate_absnorm(g5.to(dtype), 24)
    with pytest.raises(TypeError, match="float32"):
        F.absnorm_propagate(g5.repeat(1, 2, 1, 1).double(), x, 3, 5)
    with pytest.raises(TypeError, match="float32"):
        cspn_amd.Affinity_Propagate(3, 3)(g5[:, :8].double(), x[:, :1])


def test_numpy_arrays_still_raise_typeerror():
    g5, x = torch.rand(1, 24, 6, 9), torch.rand(1, 2, 6, 9)
    with pytest.raises(TypeError):
        F.cspn2d_forward_kxk_norm(g5.numpy(), x, None, 5, 3)
    with pytest.raises(TypeError):
        cspn_amd.affinity_propagate(x.numpy(), g5.half(), 5, 2)
    with pytest.raises(TypeError):
        cspn_amd.gate_absnorm(g5.numpy(), 24)
    with pytest.raises(TypeError):
        F.absnorm_propagate(g5.numpy(), x, 3, 5)


# ---- GPU ----
def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _gates(N, K, H, W, dtype, seed):
    """signed, unnormalised gates whose abs-sum stays near 1; a few of them tiny, so that float16 holds subnormal gates"""
    g = torch.randn(N, K * K - 1, H, W, device="cuda", generator=_gen(seed)) * (1.2 / (K * K - 1))
    g.view(-1)[::17] *= 1e-4
    g = g.to(dtype)
    if dtype == torch.float16:
        assert bool(((g.float().abs() < 6e-5) & (g != 0)).any())
    return g


def _values(N, C, H, W, seed):
    return torch.rand(N, C, H, W, device="cuda", generator=_gen(seed)) * 4 - 1


def _off8(t):
    """a copy of the 16-bit tensor t whose storage starts one element after an 8-byte boundary: 2-byte aligned, not 8-byte aligned"""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 == 2 and v.is_contiguous()
    return v


def _same(a, b):
    """equal where neither is NaN, NaN in the same places, same dtype"""
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0), b.masked_fill(nb, 0))


# (N, C, H, W, n, view): tiles are 16 rows x 64 columns
SHAPES = [
    (2, 1, 20, 128, 5, False),    # W % 4 == 0, 8-byte aligned gates: the 8-byte loads; two tiles each way
    (1, 3, 37, 130, 2, False),    # W % 4 == 2: the guarded scalar path; several tiles each way, C = 3
    (1, 1, 9, 13, 1, False),      # W % 4 == 1, smaller than one tile
    (1, 3, 18, 68, 24, True),     # W % 4 == 0 behind a gate pointer that is 2-byte but not 8-byte aligned; 24 steps
    (1, 1, 5, 8, 24, False),      # smaller than one tile, vector path
    (2, 3, 33, 192, 1, False),    # three tiles each way, one step
    (2, 2, 35, 196, 3, False),    # 3 x 4 tiles, two images: a grid that is not square (tests/test_kxk_tilegrid.py), vector path
    (1, 2, 67, 70, 3, False),     # 5 x 2 tiles, the guarded path
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d-n%d%s" % (s[:5] + ("-view" if s[5] else "",)))
def test_none_op_is_bitwise_the_float32_engine_on_widened_gates(dtype, K, shape):
    N, C, H, W, n, view = shape
    g = _gates(N, K, H, W, dtype, 1 + K)
    if view:
        g = _off8(g)
    x, go = _values(N, C, H, W, 2), _values(N, C, H, W, 3)
    gf = g.float()
    out = F.cspn2d_forward_kxk(g, x, K, n)
    ref = F.cspn2d_forward_kxk(gf, x, K, n)
    assert out.dtype == torch.float32 and torch.equal(out, ref)
    out_h, hist = F.cspn2d_forward_kxk(g, x, K, n, return_history=True)
    ref_h, rhist = F.cspn2d_forward_kxk(gf, x, K, n, return_history=True)
    assert torch.equal(out_h, ref) and torch.equal(ref_h, ref)
    assert n < 2 or torch.equal(hist, rhist)   # (n = 1 keeps no level: the history is an unwritten placeholder)
    gg, gx = F.cspn2d_backward_kxk(g, x, go, K, n, hist)
    rg, rx = F.cspn2d_backward_kxk(gf, x, go, K, n, rhist)
    assert gx.dtype == torch.float32 and torch.equal(gx, rx)
    assert gg.dtype == dtype and _same(gg, rg.to(dtype))
    # either gradient alone, and the history made by the backward itself
    gg2, none = F.cspn2d_backward_kxk(g, x, go, K, n, None, need_x=False)
    none2, gx2 = F.cspn2d_backward_kxk(g, x, go, K, n, None, need_gate=False)
    assert none is None and none2 is None and _same(gg2, gg) and torch.equal(gx2, gx)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_float16_gradients_in_the_subnormal_range_are_rounded_once(K):
    N, C, H, W, n = 1, 2, 19, 68, 3
    g = _gates(N, K, H, W, torch.float16, 5)
    x = _values(N, C, H, W, 6)
    go = _values(N, C, H, W, 7) * 2e-6   # dL/dgate ~ 1e-6 .. 1e-5: below float16's smallest normal 6.1e-5, above its smallest subnormal 6e-8
    gg, gx = F.cspn2d_backward_kxk(g, x, go, K, n)
    rg, rx = F.cspn2d_backward_kxk(g.float(), x, go, K, n)
    want = rg.to(torch.float16)
    sub = (want != 0) & (want.float().abs() < 6.1e-5)
    assert int(sub.sum()) > want.numel() // 2, "the case does not reach the subnormal range"
    assert torch.equal(gx, rx) and _same(gg, want)
    assert bool((gg[sub] != 0).all())   # kept, not flushed


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [5, 7])
def test_nan_and_inf_gates_land_where_the_float32_engine_puts_them(dtype, K):
    N, C, H, W, n = 1, 2, 20, 72, 2
    g = _gates(N, K, H, W, dtype, 8)
    g[0, 3, 4, 5] = float("nan")
    g[0, K * K - 2, 15, 66] = float("inf")
    g[0, 0, 17, 1] = float("-inf")
    x, go = _values(N, C, H, W, 9), _values(N, C, H, W, 10)
    out = F.cspn2d_forward_kxk(g, x, K, n)
    ref = F.cspn2d_forward_kxk(g.float(), x, K, n)
    assert bool(out.isnan().any()) and bool(out.isinf().any())
    assert torch.equal(out.isnan(), ref.isnan()) and torch.equal(out.isinf(), ref.isinf())
    gg, gx = F.cspn2d_backward_kxk(g, x, go, K, n)
    rg, rx = F.cspn2d_backward_kxk(g.float(), x, go, K, n)
    rg = rg.to(dtype)
    assert torch.equal(gx.isnan(), rx.isnan()) and torch.equal(gx.isinf(), rx.isinf())
    assert torch.equal(gg.isnan(), rg.isnan()) and torch.equal(gg.isinf(), rg.isinf())


def _norm_inputs(B, C, H, W, K, sparse, dtype, seed):
    gen = _gen(seed)
    g = torch.randn(B, K * K - 1, H, W, device="cuda", generator=gen).to(dtype)
    h = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
    s = None
    if sparse:
        sc = 1 if sparse == "shared" else C
        s = (torch.rand(B, sc, H, W, device="cuda", generator=gen) < 0.1).float() * (torch.rand(B, sc, H, W, device="cuda", generator=gen) * 10 + 0.1)
        s.view(-1)[min(3, s.numel() - 1)] = -2.5
    return g, h, s


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("sparse", [None, "shared", "per_channel"])
def test_norm_contract_is_bitwise_the_float32_engine_on_widened_guidance(dtype, K, norm, sparse):
    for (B, C, H, W, n, view) in ((1, 3, 20, 72, 3, False), (2, 3, 21, 70, 2, False), (1, 1, 7, 9, 1, False), (1, 3, 18, 68, 5, True)):
        g, h, s = _norm_inputs(B, C, H, W, K, sparse, dtype, 11 + K)
        if view:
            g = _off8(g)
        go = _values(B, C, H, W, 12)
        gf = g.float()
        out = F.cspn2d_forward_kxk_norm(g, h, s, K, n, norm)
        ref = F.cspn2d_forward_kxk_norm(gf, h, s, K, n, norm)
        assert out.dtype == torch.float32 and torch.equal(out, ref), (B, C, H, W)
        gg, gh = F.cspn2d_backward_kxk_norm(g, h, s, go, K, n, norm)
        rg, rh = F.cspn2d_backward_kxk_norm(gf, h, s, go, K, n, norm)
        assert gh.dtype == torch.float32 and torch.equal(gh, rh), (B, C, H, W)
        assert gg.dtype == dtype and _same(gg, rg.to(dtype)), (B, C, H, W)
        none, gh2 = F.cspn2d_backward_kxk_norm(g, h, s, go, K, n, norm, need_guidance=False)
        assert none is None and torch.equal(gh2, gh)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [5, 7])
def test_against_the_float64_statements(dtype, K):
    """against truth, not only against itself: the float64 torch statements evaluated on the widened gates"""
    N, C, H, W, n = 2, 2, 21, 70, 6
    g, x = _gates(N, K, H, W, dtype, 13), _values(N, C, H, W, 14)
    out = F.cspn2d_forward_kxk(g, x, K, n)
    ref = _torch_noneKxK(g.float().double().cpu(), x.double().cpu(), K, n)
    e = _rel(out.cpu().numpy(), ref.numpy())
    print("none op %s K=%d rel %.3g" % (dtype, K, e))
    assert e <= RTOL
    gd, h, s = _norm_inputs(N, C, H, W, K, "shared", dtype, 15)
    for norm in ("8sum", "8sum_abs"):
        out = F.cspn2d_forward_kxk_norm(gd, h, s, K, n, norm)
        ref = torch_kxk_norm(gd.float().double().cpu(), h.double().cpu(), s.double().cpu(), K, n, norm)
        e = _rel(out.cpu().numpy(), ref.numpy())
        print("norm %s %s K=%d rel %.3g" % (norm, dtype, K, e))
        assert e <= RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [5, 7])
def test_affinity_propagate_takes_16_bit_gates_and_values(dtype, K):
    N, C, H, W, n = 1, 3, 20, 72, 4
    g = _gates(N, K, H, W, dtype, 16).requires_grad_(True)
    x16 = _values(N, C, H, W, 17).to(dtype).requires_grad_(True)
    gf = g.detach().float().requires_grad_(True)
    xf = x16.detach().float().requires_grad_(True)
    go = _values(N, C, H, W, 18)
    out = cspn_amd.affinity_propagate(x16, g, K, n)
    ref = cspn_amd.affinity_propagate(xf, gf, K, n)
    assert out.dtype == torch.float32 and torch.equal(out, ref)
    out.backward(go)
    ref.backward(go)
    assert g.grad.dtype == dtype and _same(g.grad, gf.grad.to(dtype))
    assert x16.grad.dtype == dtype and _same(x16.grad, xf.grad.to(dtype))   # autograd's cast back through .float()
    with torch.no_grad():
        assert torch.equal(cspn_amd.affinity_propagate(x16, g, K, n), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [5, 7])
def test_module_under_autocast_reaches_the_conv(dtype, K):
    """Affinity_PropagateKxK(24, K) fed by a conv under torch.autocast: the guidance arrives in 16 bits and goes to the engine as it is.
    The float32 route widens the same guidance by hand.  Output and dL/dguidance are bitwise equal (dL/dguidance is the float32
    gradient rounded once either way: by the engine's store, or by autograd's cast back through .float()), so the conv's backward sees the
    same input twice, and with deterministic algorithms asked of the conv library it returns the same weight and bias gradients:
    torch.equal."""
    KK = K * K - 1
    B, Cin, H, W = 2, 4, 24, 72
    torch.manual_seed(20 + K)
    conv = torch.nn.Conv2d(Cin, KK, 3, padding=1).cuda()
    feat = torch.randn(B, Cin, H, W, device="cuda", generator=_gen(21))
    blur = torch.rand(B, 1, H, W, device="cuda", generator=_gen(22)) * 10
    sp = (torch.rand(B, 1, H, W, device="cuda", generator=_gen(23)) < 0.1).float() * blur
    wgt = torch.randn(B, 1, H, W, device="cuda", generator=_gen(24))
    m = cspn_amd.Affinity_PropagateKxK(24, K, "8sum")
    res = []
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True   # the conv's backward: the same algorithm, without atomics, in both routes
    for widen in (False, True):
        conv.zero_grad()
        with torch.autocast(device_type="cuda", dtype=dtype):
            guid = conv(feat)
            assert guid.dtype == dtype
            guid.retain_grad()
            out = m(guid.float() if widen else guid, blur, sp)
            assert out.dtype == torch.float32
            loss = (out * wgt).sum()
        loss.backward()
        res.append((out.detach(), guid.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()))
    torch.backends.cudnn.deterministic = det
    (o1, gg1, w1, b1), (o2, gg2, w2, b2) = res
    assert torch.equal(o1, o2)
    assert gg1.dtype == dtype and _same(gg1, gg2) and bool((gg1 != 0).any())
    for a, b in ((w1, w2), (b1, b2)):
        assert bool(a.isfinite().all()) and float(a.abs().max()) > 0
        print("conv grad %s K=%d max abs diff %.3g" % (dtype, K, float((a - b).abs().max())))
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_paths_without_a_16_bit_kernel_widen_and_return_float32(dtype):
    gen = _gen(30)
    B, H, W = 2, 24, 64
    g = torch.randn(B, 8, H, W, device="cuda", generator=gen).to(dtype)
    h = (torch.rand(B, 1, H, W, device="cuda", generator=gen) * 10).to(dtype)
    s = ((torch.rand(B, 1, H, W, device="cuda", generator=gen) < 0.1).float() * 3).to(dtype)
    with torch.no_grad():
        for m in (cspn_amd.Affinity_Propagate(24, 3, "8sum"), cspn_amd.Affinity_PropagateKxK(24, 3, "8sum_abs")):
            out = m(g, h, s)
            assert out.dtype == torch.float32 and torch.equal(out, m(g.float(), h.float(), s.float()))
        wb = cspn_amd.cspn2d_normalize(g.float(), "8sum").to(dtype)
        out = cspn_amd.propagate_prenorm(wb, h, s, 24)
        assert out.dtype == torch.float32 and torch.equal(out, cspn_amd.propagate_prenorm(wb.float(), h.float(), s.float(), 24))
        # the Paddle mirror with kernel_size 3, 2D (C = 1 and 3) and 3D
        w8 = (g.float().abs() / g.float().abs().sum(1, keepdim=True)).to(dtype)
        for C in (1, 3):
            x = torch.rand(B, C, H, W, device="cuda", generator=gen).to(dtype)
            out = cspn_amd.affinity_propagate(x, w8, 3, 4)
            assert out.dtype == torch.float32 and torch.equal(out, cspn_amd.affinity_propagate(x.float(), w8.float(), 3, 4))
        g3 = torch.rand(1, 26, 4, 12, 20, device="cuda", generator=gen)
        g3 = (g3 / g3.sum(1, keepdim=True)).to(dtype)
        x3 = torch.rand(1, 1, 4, 12, 20, device="cuda", generator=gen).to(dtype)
        out = cspn_amd.affinity_propagate(x3, g3, 3, 3)
        assert out.dtype == torch.float32 and torch.equal(out, cspn_amd.affinity_propagate(x3.float(), g3.float(), 3, 3))
        # the demo's module: 2D at 3 x 3 and 5 x 5, 3D
        for dim, ks, S in ((2, 3, (20, 36)), (2, 5, (20, 36)), (3, 3, (4, 12, 20))):
            KK = ks ** dim - 1
            guide = torch.randn(1, 2 * KK, *S, device="cuda", generator=gen).to(dtype)
            feat = torch.rand(1, 2, *S, device="cuda", generator=gen).to(dtype)
            m = cspn_amd.CSPN(dim, 2, ks, 3)
            out = m(guide, feat)
            assert out.dtype == torch.float32 and torch.equal(out, m(guide.float(), feat.float())), (dim, ks)
    # and the gradient comes back through the cast, in the input's dtype
    gr, hr = g.clone().requires_grad_(True), h.clone().requires_grad_(True)
    gf, hf = g.float().requires_grad_(True), h.float().requires_grad_(True)
    go = torch.randn(B, 1, H, W, device="cuda", generator=gen)
    m = cspn_amd.Affinity_Propagate(24, 3, "8sum")
    m(gr, hr, s).backward(go)
    m(gf, hf, s.float()).backward(go)
    assert gr.grad.dtype == dtype and _same(gr.grad, gf.grad.to(dtype)) and _same(hr.grad, hf.grad.to(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_streams_and_a_captured_graph_give_the_eager_result(dtype):
    K, N, C, H, W, n = 5, 2, 2, 40, 136, 6
    g1, g2 = _gates(N, K, H, W, dtype, 40), _gates(N, K, H, W, dtype, 41)
    x1, x2 = _values(N, C, H, W, 42), _values(N, C, H, W, 43)
    gd, h, s = _norm_inputs(N, C, H, W, 7, "shared", dtype, 44)
    r1, r2 = F.cspn2d_forward_kxk(g1, x1, K, n), F.cspn2d_forward_kxk(g2, x2, K, n)
    rn = F.cspn2d_forward_kxk_norm(gd, h, s, 7, n, "8sum")
    rg1, rx1 = F.cspn2d_backward_kxk(g1, x1, x2, K, n)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            o1 = F.cspn2d_forward_kxk(g1, x1, K, n)
            b1 = F.cspn2d_backward_kxk(g1, x1, x2, K, n)
        with torch.cuda.stream(s2):
            o2 = F.cspn2d_forward_kxk(g2, x2, K, n)
            on = F.cspn2d_forward_kxk_norm(gd, h, s, 7, n, "8sum")
        torch.cuda.synchronize()
        assert torch.equal(o1, r1) and torch.equal(o2, r2) and torch.equal(on, rn)
        assert _same(b1[0], rg1) and torch.equal(b1[1], rx1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c1 = F.cspn2d_forward_kxk(g1, x1, K, n)
        cn = F.cspn2d_forward_kxk_norm(gd, h, s, 7, n, "8sum")
        cg, cx = F.cspn2d_backward_kxk(g1, x1, x2, K, n)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c1, r1) and torch.equal(cn, rn) and _same(cg, rg1) and torch.equal(cx, rx1)
    # new contents behind the captured pointers
    g1.copy_(g2)
    x1.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c1, r2)
