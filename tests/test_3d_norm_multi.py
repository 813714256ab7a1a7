"""C value channels on SHARED 3D guidance in the normalising / masked modes (cspn3d_forward_norm_multi_f32 / cspn3d_backward_norm_multi_f32 and
their _g16 forms, cspn_amd.cspn3d_forward_norm / cspn3d_backward_norm with feat [B,C,D,H,W], cspn_amd.Affinity_Propagate3d on a cost volume).
CPU: a plain-torch float64 statement of the C-channel forward (tests/test_backward3d_norm.py::_statement's equations with the channels
     broadcast over the shared w' and coef), pinned channel by channel to oracle/cspn_oracle.c's 3D forward; the ABI's exports, argument
     checks and workspace queries; a float32 numpy restatement of the backward formulas of include/cspn_amd.h.
GPU: the HIP results against float64 autograd through that statement, element-wise, and their properties."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import cspn3d_oracle
from oracle.backward import OFF3

# the project's gradient check (tests/test_backward3d_norm.py: rtol 2e-4 element-wise above a floor of GFLOOR max|ref|).  Nobody had measured
# the floor with the sum over the channels in dwb_k = u (dW'_k - sum_c dC_c H_{0,c}), so _backward_np32 below -- float32 numpy, the formulas of
# include/cspn_amd.h -- was run on a CPU against the float64 autograd on every case of CASES + FUSED_CASES, both norms, the three masks, before
# any HIP result existed.  The floor each result needs (the smallest atol_frac at which helpers.assert_close passes with rtol 2e-4):
#   worst: 2.23e-6 max|ref| for grad_guidance (1.28e-6 for grad_feat) at (2,6,10,36), n = 12, C = 2, no mask, either norm (unsigned gates
#   there), max-norm error 6.3e-6; the fused shapes need at most 1.4e-6 ((1,9,17,72), n = 5, C = 3, '8sum_abs', no mask), every masked and
#   every small case under 7.4e-7.
# That is under half of the project's 1.24e-5 (tests/test_backward3d_norm.py's GFLOOR), so the project's figure is kept
GFLOOR = 1.24e-5
GTOL = 2e-4

NORMS = ("8sum", "8sum_abs")
MASKS = ("nomask", "mask", "mask_neg")
# (B, D, H, W), n_iter, C
CASES = [((2, 4, 5, 7), 1, 3),      # odd W: the scalar kernels, with batch and channel strides
         ((1, 3, 6, 8), 4, 2),      # the vector kernels
         ((2, 6, 10, 36), 12, 2),   # many levels, several workgroups
         ((1, 1, 1, 4), 3, 2),      # one quad is the whole volume
         ((2, 1, 2, 3), 3, 3)]      # every z-neighbour out of range
# algo 'persistent' must take the forward and the backward here
FUSED_CASES = [((1, 8, 8, 64), 3, 2),    # one tile
               ((1, 9, 17, 72), 5, 3)]   # partial tiles


def _shift(a, off, dims):
    """out(p) = a(p + off), zero outside; a: [..., D, H, W]"""
    (dz, dy, dx), (D, H, W) = off, dims
    pad = torch.nn.functional.pad(a, (1, 1, 1, 1, 1, 1))
    return pad[..., 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def _statement(g, feat, sparse, n_iter, norm):
    """the C-channel forward in plain torch ops (autograd-able), in the dtype of its inputs: g [B,26,D,H,W], feat [B,C,D,H,W], sparse None or
    [B,1,D,H,W] shared by the channels -> [B,C,D,H,W]"""
    dims = tuple(g.shape[2:])
    if norm == "none":
        wb = [g[:, k] for k in range(26)]
        sigma = None
    else:
        gt = g.abs() if norm == "8sum_abs" else g
        G = [_shift(gt[:, k], OFF3[k], dims) for k in range(26)]
        S = sum(x.abs() for x in G)
        wb = [x / S for x in G]
        sigma = sum(wb)
    m = torch.sign(sparse[:, 0]) if sparse is not None else torch.zeros_like(g[:, 0])
    u = 1 - m
    w = [(u * x)[:, None] for x in wb]                                    # shared: [B,1,D,H,W]
    coef = (m if sigma is None else u * (1 - sigma) + m)[:, None]
    x = feat
    for _ in range(n_iter):
        x = coef * feat + sum(w[k] * _shift(x, OFF3[k], dims) for k in range(26))
    return x


def _inputs(shape, C, seed, signed=True, mask="nomask"):
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    g = torch.rand(B, 26, D, H, W, generator=gen)
    if signed:
        g = g - 0.3
    feat = torch.rand(B, C, D, H, W, generator=gen)
    go = torch.randn(B, C, D, H, W, generator=gen)
    sparse = None
    if mask != "nomask":
        sparse = (torch.rand(B, 1, D, H, W, generator=gen) < 0.2).float() * (feat[:, :1] + 0.1)
        sparse.view(-1)[0] = 1.5   # at least one pinned voxel at every size
        if mask == "mask_neg":
            sparse.view(-1)[-1] = -2.0   # m = -1, u = 2
    return g, feat, sparse, go


@functools.lru_cache(maxsize=None)
def _case(shape, n_iter, C, norm, mask):
    """inputs, the float64 forward and its autograd gradients of one case, computed once and shared (read-only)"""
    g, feat, sparse, go = _inputs(shape, C, 29 + n_iter, signed=n_iter != 12, mask=mask)
    gd, fd = g.double().requires_grad_(True), feat.double().requires_grad_(True)
    out = _statement(gd, fd, None if sparse is None else sparse.double(), n_iter, norm)
    out.backward(go.double())
    return g, feat, sparse, go, out.detach().numpy(), gd.grad.numpy(), fd.grad.numpy()


def _backward_np32(g, feat, sparse, go, n_iter, norm):
    """the backward formulas of include/cspn_amd.h in float32 numpy (norm '8sum' / '8sum_abs'): -> (grad_guidance, grad_feat)"""
    f32 = np.float32
    g, feat, go = (np.asarray(t, f32) for t in (g, feat, go))
    B, C, D, H, W = feat.shape

    def shift(a, off):
        dz, dy, dx = off
        pad = np.zeros(a.shape[:-3] + (D + 2, H + 2, W + 2), f32)
        pad[..., 1:-1, 1:-1, 1:-1] = a
        return pad[..., 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    neg = lambda off: tuple(-o for o in off)
    gt = np.abs(g) if norm == "8sum_abs" else g
    G = np.stack([shift(gt[:, k], OFF3[k]) for k in range(26)], 1)
    S = np.abs(G).sum(1, dtype=f32)
    wb = G / S[:, None]
    sigma = wb.sum(1, dtype=f32)
    m = np.sign(np.asarray(sparse, f32)[:, 0]) if sparse is not None else np.zeros_like(S)
    u = f32(1) - m
    w = u[:, None] * wb
    coef = u * (f32(1) - sigma) + m
    Hs = [feat]
    for _ in range(n_iter - 1):
        nxt = coef[:, None] * feat
        for k in range(26):
            nxt = nxt + w[:, k, None] * shift(Hs[-1], OFF3[k])
        Hs.append(nxt.astype(f32))
    A = go
    dW = np.zeros_like(w)
    dC = np.zeros_like(feat)
    for t in range(n_iter - 1, -1, -1):   # A = A_{t+1}
        dC = dC + A
        for k in range(26):
            dW[:, k] += (A * shift(Hs[t], OFF3[k])).sum(1, dtype=f32)
        nxt = np.zeros_like(A)
        for k in range(26):
            nxt = nxt + shift(w[:, k, None] * A, neg(OFF3[k]))
        A = nxt.astype(f32)
    gf = A + dC * coef[:, None]
    Dh = (dC * feat).sum(1, dtype=f32)
    dwb = u[:, None] * (dW - Dh[:, None])
    T = (dwb * G).sum(1, dtype=f32) / (S * S)
    dG = dwb / S[:, None] - np.sign(G) * T[:, None]
    gg = np.stack([shift(dG[:, k], neg(OFF3[k])) for k in range(26)], 1)
    if norm == "8sum_abs":
        gg = gg * np.sign(g)
    return gg.astype(f32), gf.astype(f32)


def _check(a, b, what=""):
    from helpers import assert_close
    return assert_close(a, b, what, rtol=GTOL, atol_frac=GFLOOR)


def _err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _cuda1(t):
    return None if t is None else t.cuda()


def _cuda(*ts):
    return tuple(_cuda1(t) for t in ts)


def _off_by_one_float(t):
    """t on the GPU as a contiguous view whose pointer is 4 bytes off a 16-byte boundary"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS + ("none",))
@pytest.mark.parametrize("mask", ("nomask", "mask_neg"))
@pytest.mark.parametrize("shape,n_iter,C", [((2, 4, 5, 7), 1, 3), ((1, 3, 6, 8), 4, 2)])
def test_each_channel_of_the_float64_statement_is_the_oracles_forward(shape, n_iter, C, norm, mask):
    g, feat, sparse, _ = _inputs(shape, C, 5 + n_iter, mask=mask)
    got = _statement(g.double(), feat.double(), None if sparse is None else sparse.double(), n_iter, norm).numpy()
    assert got.shape == (shape[0], C) + shape[1:]
    for c in range(C):
        ref = cspn3d_oracle(g.numpy(), feat[:, c:c + 1].contiguous().numpy(), None if sparse is None else sparse.numpy(), n_iter, norm)
        from helpers import assert_close
        assert_close(got[:, c:c + 1], ref, "channel %d" % c)
        assert _err(got[:, c:c + 1], ref) <= 1e-6


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape,n_iter,C", [((2, 4, 5, 7), 1, 3), ((1, 3, 6, 8), 4, 2), ((2, 1, 2, 3), 3, 3)])
def test_float32_restatement_of_the_backward_formulas(shape, n_iter, C, norm, mask):
    """the formulas of include/cspn_amd.h, in float32 on the CPU, against the float64 autograd: under HALF the gradient bound (the measurement
    that settled GFLOOR ran this on every GPU case)"""
    from helpers import assert_close
    g, feat, sparse, go, _, dG, dF = _case(shape, n_iter, C, norm, mask)
    gg, gf = _backward_np32(g.numpy(), feat.numpy(), None if sparse is None else sparse.numpy(), go.numpy(), n_iter, norm)
    assert_close(gg, dG, "grad_guidance", rtol=GTOL, atol_frac=GFLOOR / 2)
    assert_close(gf, dF, "grad_feat", rtol=GTOL, atol_frac=GFLOOR / 2)


SYMBOLS = ("cspn3d_forward_norm_multi_workspace_bytes", "cspn3d_forward_norm_multi_f32", "cspn3d_forward_norm_multi_g16",
           "cspn3d_backward_norm_multi_workspace_bytes", "cspn3d_backward_norm_multi_f32", "cspn3d_backward_norm_multi_g16")


def test_symbols_are_exported_declared_and_bound():
    import cspn_amd
    from cspn_amd import _lib
    lib = cspn_amd.load()
    assert lib.cspn_abi_version() == 5
    header = open(os.path.join(os.path.dirname(os.path.abspath(cspn_amd.__file__)), "..", "include", "cspn_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name + "(" in header and _lib.symbol(name) is not None, name
    assert "#define CSPN_ABI_VERSION 5" in header


def test_abi_argument_errors_before_any_launch():
    import cspn_amd
    from cspn_amd import _lib
    cspn_amd.load()
    fwd, bwd = _lib.symbol("cspn3d_forward_norm_multi_f32"), _lib.symbol("cspn3d_backward_norm_multi_f32")
    fwd16, bwd16 = _lib.symbol("cspn3d_forward_norm_multi_g16"), _lib.symbol("cspn3d_backward_norm_multi_g16")
    qf, qb = _lib.symbol("cspn3d_forward_norm_multi_workspace_bytes"), _lib.symbol("cspn3d_backward_norm_multi_workspace_bytes")
    BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
    B, C, D, H, W = 1, 2, 2, 2, 4
    err = lambda: cspn_amd.load().cspn_last_error()
    # never dereferenced: every call below returns before a launch.  Far apart, so that no range overlaps another
    guid, feat, sparse, gout, gg, gf, ws, out = (ctypes.c_void_p((i + 1) << 32) for i in range(8))

    def back(n_iter=2, norm=1, algo=0, dims=(B, C, D, H, W), ws_bytes=1 << 30, outs=(gg, gf), sp=sparse, w=ws, gd=guid):
        return bwd(gd, feat, sp, gout, outs[0], outs[1], *dims, n_iter, norm, algo, w, ws_bytes, None)

    def forw(n_iter=2, norm=1, algo=0, dims=(B, C, D, H, W), ws_bytes=1 << 30, o=out, sp=sparse, w=ws, gd=guid):
        return fwd(gd, feat, sp, o, *dims, n_iter, norm, algo, w, ws_bytes, None)

    for run in (back, forw):
        assert run(norm=3) == BADARG and b"norm_type" in err()   # PRENORM
        assert run(norm=7) == BADARG and run(norm=-1) == BADARG
        assert run(algo=5) == BADARG
        assert run(dims=(0, C, D, H, W)) == 0
        assert run(dims=(-1, C, D, H, W)) == BADARG and run(dims=(B, 0, D, H, W)) == BADARG and run(dims=(B, C, 0, H, W)) == BADARG
        assert run(dims=(B, C, D, H, -3)) == BADARG
        assert run(n_iter=-1) == BADARG
        assert run(gd=None) == BADARG
        assert run(w=ctypes.c_void_p((7 << 32) + 64)) == WORKSPACE   # not 256-byte aligned
        assert run(algo=2) == UNSUPPORTED and b"persistent" in err()   # a volume of one quad a row: 'auto' would not fuse
    need = qb(B, C, D, H, W, 2, 1, 1)
    assert need > 0 and back(ws_bytes=need - 1) == WORKSPACE and b"workspace" in err() and back(ws_bytes=need, outs=(None, None)) == 0
    need = qf(B, C, D, H, W, 2, 1, 1)
    assert need > 0 and forw(ws_bytes=need - 1) == WORKSPACE and b"workspace" in err()
    # an output on top of an input, of the other output or of the workspace
    assert back(outs=(guid, gf)) == BADARG and back(outs=(gg, feat)) == BADARG and back(outs=(gg, sparse)) == BADARG
    assert back(outs=(gg, gg)) == BADARG and back(outs=(gg, ws)) == BADARG and back(outs=(gout, None)) == BADARG
    assert b"overlap" in err()
    assert forw(o=guid) == BADARG and forw(o=feat) == BADARG and forw(o=sparse) == BADARG and forw(o=ws) == BADARG and b"overlap" in err()
    assert back(outs=(None, None)) == 0 and back(n_iter=0, outs=(None, None)) == 0   # nothing asked for: nothing launched
    # the 16-bit forms: the dtype and the 16-bit tensors' addresses first
    assert fwd16(guid, 3, feat, sparse, out, B, C, D, H, W, 2, 1, 0, ws, 1 << 30, None) == BADARG and b"gate_dtype" in err()
    assert bwd16(guid, 0, feat, sparse, gout, gg, gf, B, C, D, H, W, 2, 1, 0, ws, 1 << 30, None) == BADARG
    assert bwd16(ctypes.c_void_p((1 << 32) + 1), 1, feat, sparse, gout, gg, gf, B, C, D, H, W, 2, 1, 0, ws, 1 << 30, None) == BADARG
    assert bwd16(guid, 2, feat, sparse, gout, gg, gf, B, C, D, H, W, 2, 3, 0, ws, 1 << 30, None) == BADARG   # PRENORM
    assert fwd16(guid, 1, feat, sparse, out, B, C, D, H, W, 2, 1, 0, ws, 16, None) == WORKSPACE


def test_workspace_queries():
    import cspn_amd
    from cspn_amd import _lib
    cspn_amd.load()
    qf, qb = _lib.symbol("cspn3d_forward_norm_multi_workspace_bytes"), _lib.symbol("cspn3d_backward_norm_multi_workspace_bytes")
    for q in (qf, qb):
        assert q(0, 2, 4, 8, 16, 2, 1, 0) == 0 and q(2, 0, 4, 8, 16, 2, 1, 0) == 0 and q(2, 2, 4, 8, -1, 2, 1, 0) == 0
        assert q(2, 2, 4, 8, 16, 0, 1, 0) == 0 and q(2, 2, 4, 8, 16, 2, 3, 0) == 0 and q(2, 2, 4, 8, 16, 2, -1, 0) == 0
    # C = 1: the single-channel queries
    for norm in (0, 1, 2):
        for sp in (0, 1):
            for dims, n in (((2, 4, 8, 16), 3), ((1, 3, 5, 7), 1), ((1, 8, 8, 64), 12)):
                assert qf(dims[0], 1, *dims[1:], n, norm, sp) == _lib.symbol("cspn3d_workspace_bytes_ex")(*dims, n, norm, sp)
                assert qb(dims[0], 1, *dims[1:], n, norm, sp) == _lib.symbol("cspn3d_backward_norm_g16_workspace_bytes")(*dims, n, norm, sp)
                if norm != 2 or sp:
                    assert qb(dims[0], 1, *dims[1:], n, norm, sp) == _lib.symbol("cspn3d_backward_norm_workspace_bytes")(*dims, n, norm, sp)
    # C > 1: w' (26 planes) and coef once, the levels [level][B][C][V] for H and for A
    vol = 2 * 4 * 8 * 16 * 4
    sizes = [qb(2, 3, 4, 8, 16, n, 1, 1) for n in range(1, 8)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] >= 27 * vol + 3 * vol
    assert sizes[2] - sizes[0] == 4 * 3 * vol   # two value and two adjoint levels of C volumes more
    assert qb(2, 3, 4, 8, 16, 3, 2, 0) == _lib.symbol("cspn3d_backward_multi_g16_workspace_bytes")(2, 3, 4, 8, 16, 3)   # the Paddle contract
    assert qf(2, 3, 4, 8, 16, 3, 1, 1) >= 27 * vol + 2 * 3 * vol
    assert qf(2, 3, 4, 8, 16, 3, 2, 0) >= _lib.symbol("cspn3d_workspace_bytes_ex")(2, 4, 8, 16, 3, 2, 0)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _fwd(args, n_iter, norm, algo="auto"):
    import cspn_amd
    return cspn_amd.cspn3d_forward_norm(args[0], args[1], args[2], n_iter, norm, algo)


def _bwd(args, n_iter, norm, algo="auto", **kw):
    import cspn_amd
    return cspn_amd.cspn3d_backward_norm(*args, n_iter, norm, algo, **kw)


def _parity(shape, n_iter, C, norm, mask, place=_cuda1, algo="auto"):
    from helpers import assert_close
    g, feat, sparse, go, ref, dG, dF = _case(shape, n_iter, C, norm, mask)
    args = tuple(place(t) for t in (g, feat, sparse, go))
    what = "%s C=%d %s %s n=%d %s" % (shape, C, norm, mask, n_iter, algo)
    out = _fwd(args, n_iter, norm, algo)
    err, worst = assert_close(out.cpu().numpy(), ref, "out " + what)
    print("out %s: max-norm rel err %.3g, element-wise excess %.3g" % (what, err, worst))
    gg, gf = _bwd(args, n_iter, norm, algo)
    for name, got, want in (("grad_guidance", gg, dG), ("grad_feat", gf, dF)):
        err, worst = _check(got.cpu().numpy(), want, "%s %s" % (name, what))
        print("%s %s: max-norm rel err %.3g, element-wise excess %.3g" % (name, what, err, worst))
    return args, out, gg, gf


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,n_iter,C", CASES + FUSED_CASES)
def test_hip_vs_float64_autograd(shape, n_iter, C, norm, mask):
    """out under helpers.assert_close's defaults; the gradients element-wise |got - ref| <= GFLOOR max|ref| + GTOL |ref| and max-norm <= GTOL"""
    import cspn_amd
    args, out, gg, gf = _parity(shape, n_iter, C, norm, mask)
    # either output alone: bitwise
    gg1, none = _bwd(args, n_iter, norm, need_feat=False)
    none2, gf1 = _bwd(args, n_iter, norm, need_guidance=False)
    assert none is None and none2 is None and torch.equal(gg1, gg) and torch.equal(gf1, gf)
    if (shape, n_iter, C) in FUSED_CASES:
        # 'persistent' must take both ways here, and is what 'auto' ran; one launch per step within the same bounds
        assert torch.equal(_fwd(args, n_iter, norm, "persistent"), out)
        ggp, gfp = _bwd(args, n_iter, norm, "persistent")
        assert torch.equal(ggp, gg) and torch.equal(gfp, gf)
        _parity(shape, n_iter, C, norm, mask, algo="stepwise")
    else:
        for call in (_fwd, _bwd):
            with pytest.raises(cspn_amd.CspnError, match="persistent 3D kernel does not take"):
                call(args, n_iter, norm, "persistent")
        assert torch.equal(_fwd(args, n_iter, norm, "stepwise"), out)
        ggs, gfs = _bwd(args, n_iter, norm, "stepwise")
        assert torch.equal(ggs, gg) and torch.equal(gfs, gf)
    cspn_amd.cspn3d_check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", ("nomask", "mask_neg"))
@pytest.mark.parametrize("norm", NORMS + ("none",))
@pytest.mark.parametrize("shape,n_iter", [((2, 4, 5, 7), 1), ((1, 3, 6, 8), 4), ((1, 8, 8, 64), 3)])
def test_one_channel_is_the_single_channel_entry_point_bitwise(shape, n_iter, norm, mask):
    """C = 1 through the multi-channel entry points of the C ABI: the single-channel results, bit for bit"""
    import cspn_amd
    from cspn_amd import _lib
    B, D, H, W = shape
    g, feat, sparse, go = _cuda(*_inputs(shape, 1, 3, mask=mask))
    want_out = cspn_amd.cspn3d_forward(g, feat, sparse, n_iter, norm)
    want_gg, want_gf = (cspn_amd.cspn3d_backward_norm(g, feat, sparse, go, n_iter, norm))
    ptr = lambda t: None if t is None else t.data_ptr()
    nrm, sp = _lib.NORM_TYPES[norm], int(sparse is not None)
    st = torch.cuda.current_stream().cuda_stream
    out, gg, gf = torch.empty_like(feat), torch.empty_like(g), torch.empty_like(feat)
    n = _lib.symbol("cspn3d_forward_norm_multi_workspace_bytes")(B, 1, D, H, W, n_iter, nrm, sp)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.symbol("cspn3d_forward_norm_multi_f32")(ptr(g), ptr(feat), ptr(sparse), ptr(out), B, 1, D, H, W, n_iter, nrm, 0, ws.data_ptr(), n,
                                                            st), "forward")
    n = _lib.symbol("cspn3d_backward_norm_multi_workspace_bytes")(B, 1, D, H, W, n_iter, nrm, sp)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.symbol("cspn3d_backward_norm_multi_f32")(ptr(g), ptr(feat), ptr(sparse), ptr(go), ptr(gg), ptr(gf), B, 1, D, H, W, n_iter, nrm, 0,
                                                             ws.data_ptr(), n, st), "backward")
    cspn_amd.cspn3d_check_status()
    assert torch.equal(out, want_out) and torch.equal(gg, want_gg) and torch.equal(gf, want_gf)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ("stepwise", "auto"))
def test_two_calls_with_the_same_algo_are_bitwise_equal(algo):
    import cspn_amd
    shape, n_iter, C = FUSED_CASES[1]
    args = _cuda(*_inputs(shape, C, 7, mask="mask"))
    a = (_fwd(args, n_iter, "8sum_abs", algo),) + _bwd(args, n_iter, "8sum_abs", algo)
    b = (_fwd(args, n_iter, "8sum_abs", algo),) + _bwd(args, n_iter, "8sum_abs", algo)
    cspn_amd.cspn3d_check_status()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n_iter,C", [CASES[0], CASES[1], FUSED_CASES[1]])
def test_permuting_the_channels_permutes_out_and_grad_feat_bitwise(shape, n_iter, C):
    import cspn_amd
    g, feat, sparse, go = _cuda(*_inputs(shape, C, 11, mask="mask_neg"))
    perm = list(range(1, C)) + [0]
    out, (gg, gf) = _fwd((g, feat, sparse), n_iter, "8sum"), _bwd((g, feat, sparse, go), n_iter, "8sum")
    fp, gop = feat[:, perm].contiguous(), go[:, perm].contiguous()
    outp, (ggp, gfp) = _fwd((g, fp, sparse), n_iter, "8sum"), _bwd((g, fp, sparse, gop), n_iter, "8sum")
    cspn_amd.cspn3d_check_status()
    assert torch.equal(outp, out[:, perm]) and torch.equal(gfp, gf[:, perm])
    _check(ggp.cpu().numpy(), gg.cpu().numpy(), "grad_guidance: the sum over the channels in another order")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n_iter,C", [CASES[0], ((1, 3, 6, 8), 4, 3), FUSED_CASES[1]])
def test_a_channel_with_zero_grad_out_adds_nothing(shape, n_iter, C):
    import cspn_amd
    assert C == 3
    g, feat, sparse, go = _cuda(*_inputs(shape, C, 13, mask="mask"))
    go[:, 1] = 0
    gg, gf = _bwd((g, feat, sparse, go), n_iter, "8sum_abs")
    keep = [0, 2]
    gg2, gf2 = _bwd((g, feat[:, keep].contiguous(), sparse, go[:, keep].contiguous()), n_iter, "8sum_abs")
    cspn_amd.cspn3d_check_status()
    assert not gf[:, 1].any()   # A_t = 0 at every level, dC = 0
    assert torch.equal(gf[:, keep], gf2)
    _check(gg.cpu().numpy(), gg2.cpu().numpy(), "grad_guidance without the silent channel")


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape,n_iter,C", [CASES[0], CASES[1], FUSED_CASES[0]])
def test_grad_guidance_is_the_sum_of_the_single_channel_calls(shape, n_iter, C, mask):
    import cspn_amd
    g, feat, sparse, go = _cuda(*_inputs(shape, C, 19, mask=mask))
    gg, gf = _bwd((g, feat, sparse, go), n_iter, "8sum_abs")
    loop = [cspn_amd.cspn3d_backward_norm(g, feat[:, c:c + 1].contiguous(), sparse, go[:, c:c + 1].contiguous(), n_iter, "8sum_abs") for c in range(C)]
    cspn_amd.cspn3d_check_status()
    _check(gg.cpu().numpy(), sum(x[0].double() for x in loop).cpu().numpy(), "grad_guidance against the loop")
    _check(gf.cpu().numpy(), torch.cat([x[1] for x in loop], 1).cpu().numpy(), "grad_feat against the loop")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("shape,n_iter,C", [CASES[0], CASES[1], FUSED_CASES[0]])
def test_16_bit_guidance_is_the_float32_call_on_the_widened_guidance(shape, n_iter, C, norm, dtype):
    import cspn_amd
    g, feat, sparse, go = _cuda(*_inputs(shape, C, 23, mask="mask_neg"))
    g16 = g.to(dtype)
    for algo in ("auto", "stepwise"):
        out = _fwd((g16, feat, sparse), n_iter, norm, algo)
        gg, gf = _bwd((g16, feat, sparse, go), n_iter, norm, algo)
        want = _fwd((g16.float(), feat, sparse), n_iter, norm, algo)
        wgg, wgf = _bwd((g16.float(), feat, sparse, go), n_iter, norm, algo)
        assert out.dtype == torch.float32 and gf.dtype == torch.float32 and gg.dtype == dtype
        assert torch.equal(out, want) and torch.equal(gf, wgf)
        assert torch.equal(gg.view(torch.int16), wgg.to(dtype).view(torch.int16))
    cspn_amd.cspn3d_check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("norm", NORMS)
def test_misaligned_views_take_the_scalar_kernels(norm, mask):
    """a shape of the 16-byte kernels behind pointers one float off: same bounds"""
    shape, n_iter, C = CASES[1]
    _parity(shape, n_iter, C, norm, mask, place=_off_by_one_float)


@pytest.mark.gpu
def test_norm_none_without_a_mask_is_the_paddle_contract():
    import cspn_amd
    from helpers import assert_close
    # a shape the persistent kernel declines: the per-step kernels with coef = 0, against float64
    shape, n_iter, C = (1, 3, 6, 8), 4, 2
    g, feat, _, go = _inputs(shape, C, 31)
    g = g / g.abs().sum(1, keepdim=True)
    gd, fd = g.double().requires_grad_(True), feat.double().requires_grad_(True)
    ref = _statement(gd, fd, None, n_iter, "none")
    ref.backward(go.double())
    gc, fc, goc = _cuda(g, feat, go)
    assert not cspn_amd._lib.symbol("cspn3d_multi_supported")(*((shape[0], C) + shape[1:]), n_iter)
    assert_close(_fwd((gc, fc, None), n_iter, "none").cpu().numpy(), ref.detach().numpy(), "out")
    gg, gf = _bwd((gc, fc, None, goc), n_iter, "none")
    _check(gg.cpu().numpy(), gd.grad.numpy(), "grad_gate")
    _check(gf.cpu().numpy(), fd.grad.numpy(), "grad_feat")
    want = cspn_amd.cspn3d_backward_multi(gc, fc, goc, n_iter)
    assert torch.equal(gg, want[0]) and torch.equal(gf, want[1])
    # a shape it takes: cspn3d_forward_multi / cspn3d_backward_multi, bitwise
    shape, n_iter, C = FUSED_CASES[0]
    g, feat, _, go = _inputs(shape, C, 37)
    gc, fc, goc = _cuda(g / g.abs().sum(1, keepdim=True), feat, go)
    assert cspn_amd._lib.symbol("cspn3d_multi_supported")(*((shape[0], C) + shape[1:]), n_iter)
    assert torch.equal(_fwd((gc, fc, None), n_iter, "none"), cspn_amd.cspn3d_forward_multi(gc, fc, n_iter))
    assert torch.equal(_fwd((gc, fc, None), n_iter, "none", "persistent"), cspn_amd.cspn3d_forward_multi(gc, fc, n_iter))
    gg, gf = _bwd((gc, fc, None, goc), n_iter, "none")
    want = cspn_amd.cspn3d_backward_multi(gc, fc, goc, n_iter)
    assert torch.equal(gg, want[0]) and torch.equal(gf, want[1])
    cspn_amd.cspn3d_check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("per_channel_mask", (False, True))
@pytest.mark.parametrize("norm", NORMS)
def test_module_trains_a_cost_volume_through_the_engine(norm, per_channel_mask):
    """Affinity_Propagate3d on blur_depth [1,2,3,6,8]: a shared mask is one engine call each way, a [B,C,...] mask the loop over the channels"""
    import cspn_amd
    from helpers import assert_close
    shape, n_iter, C = (1, 3, 6, 8), 4, 2
    g, feat, sparse, go = _inputs(shape, C, 41, mask="mask")
    if per_channel_mask:
        other = _inputs(shape, C, 43, mask="mask_neg")[2]
        sparse = torch.cat([sparse, other], 1)
    gd, fd = g.double().requires_grad_(True), feat.double().requires_grad_(True)
    if per_channel_mask:
        ref = torch.cat([_statement(gd, fd[:, c:c + 1], sparse[:, c:c + 1].double(), n_iter, norm) for c in range(C)], 1)
    else:
        ref = _statement(gd, fd, sparse.double(), n_iter, norm)
    ref.backward(go.double())
    m = cspn_amd.Affinity_Propagate3d(n_iter, 3, norm)
    gc, fc, sc, goc = _cuda(g, feat, sparse, go)
    g1, f1 = gc.clone().requires_grad_(True), fc.clone().requires_grad_(True)
    out = m(g1, f1, sc)
    assert out.shape == fc.shape
    assert_close(out.detach().cpu().numpy(), ref.detach().numpy(), "module out")
    (out * goc).sum().backward()
    _check(g1.grad.cpu().numpy(), gd.grad.numpy(), "module grad_guidance")
    _check(f1.grad.cpu().numpy(), fd.grad.numpy(), "module grad_blur_depth")
    if not per_channel_mask:
        assert torch.equal(out, cspn_amd.cspn3d_forward_norm(gc, fc, sc, n_iter, norm))
    cspn_amd.cspn3d_check_status()


# ---- memory hygiene, in the manner of tests/test_memory_hygiene.py: guard bands around every output and the workspace, poisoned, then stale ----
HYGIENE = {"scalar": CASES[0], "vector": CASES[1], "fused": FUSED_CASES[1]}


def _hygiene_call(n_iter):
    def call(g, feat, sparse, go):
        from cspn_amd import functional as F
        return (F.cspn3d_forward_norm(g, feat, sparse, n_iter, "8sum_abs"),) + F.cspn3d_backward_norm(g, feat, sparse, go, n_iter, "8sum_abs")
    return call


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ("zero", "ones", "big"))
@pytest.mark.parametrize("route", list(HYGIENE))
def test_poisoned_workspace_and_outputs_between_guard_bands(route, poison):
    import cspn_amd
    import memguard
    shape, n_iter, C = HYGIENE[route]
    inputs = _cuda(*_inputs(shape, C, 47, mask="mask"))
    call = _hygiene_call(n_iter)
    plane = 4 * shape[0] * C * shape[1] * shape[2] * shape[3]
    with contextlib.ExitStack() as stack:   # guarded first: an overrun shows in a band before anything runs on plain allocations
        outs, session = memguard.run_guarded(stack, poison, call, inputs, "cuda", plane)
        assert len(session.workspaces) == 2
    cspn_amd.cspn3d_check_status()
    clean = call(*inputs)
    cspn_amd.cspn3d_check_status()
    memguard.assert_same_outputs(outs, clean, "poison %r" % poison)
    for t in outs:
        assert torch.isfinite(t).all()


@pytest.mark.gpu
def test_stale_workspace_one_arena():
    import cspn_amd
    import memguard
    steps = []
    for route in ("fused", "vector", "scalar", "fused"):
        shape, n_iter, C = HYGIENE[route]
        steps.append((route, _hygiene_call(n_iter), _cuda(*_inputs(shape, C, 53 + len(steps), mask="mask_neg")), shape, C))
    plane = max(4 * s[3][0] * s[4] * s[3][1] * s[3][2] * s[3][3] for s in steps)
    sizes = []
    with contextlib.ExitStack() as stack:
        session = memguard.patched(stack, "zero", plane_bytes=plane)
        for _, call, inputs, _, _ in steps:
            call(*inputs)
            session.check()
        sizes = [n for _, n in session.workspaces]
    clean = [call(*inputs) for _, call, inputs, _, _ in steps]
    cspn_amd.cspn3d_check_status()
    arena = memguard.Arena(max(sizes), "cuda", plane)
    with contextlib.ExitStack() as stack:
        session = memguard.patched(stack, "stale", arena=arena, plane_bytes=plane)
        for i, (label, call, inputs, _, _) in enumerate(steps):
            snap = memguard.snapshot(*inputs)
            outs = call(*inputs)
            session.check()
            snap.assert_unchanged()
            cspn_amd.cspn3d_check_status()
            memguard.assert_same_outputs(outs, clean[i], "step %d (%s) in the stale arena" % (i + 1, label))
        assert arena.taken == 2 * len(steps)
