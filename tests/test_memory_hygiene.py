"""Memory hygiene of every engine call (tests/memguard.py): a call writes only inside its outputs and inside the workspace its size query promised,
its result does not depend on what the workspace, the output or the history buffer held before, and it writes no input.

Every buffer of the front-end is uninitialised caching-allocator memory (cspn_amd/functional.py: _workspace, torch.empty, torch.empty_like), so
in a test process it is mostly fresh and often zero, and in a training run it holds the previous step's data.  Here every such buffer sits between
two guard bands of 0xA5 and is filled with a poison first:
    zero   0x00                       the nearest to what the suite sees today
    ones   0xFF                       NaN in float32 / fp16 / bf16, 0xFFFFFFFF as a tag or an index
    big    float32 0x7F7FFFFF         finite, and it survives a multiplication by zero only as zero -- an addition shows it
    stale  one arena, never refilled  what the calls before left (the sequence tests at the end)

CASES is the table: one case per path an entry point dispatches to, at the smallest shape at which the path is still the one named (taken from the
parametrisations of the test that pins that path's arithmetic: `pinned`).  Where an entry point dispatches on the shape, the case asserts first that the
intended path is taken, by the library's own queries (cspn2d_auto_algo, the ring query of the hook library, cspn2d_history_bytes[_multi] for the
checkpointed ring backward, cspn2d_multi_supported, cspn3d_multi_supported for the persistent kernel, the 16-bit backward workspace query for the 3D
fused sweeps, train_utils._head_path) or, for a module, on the autograd node of its output.  Cases whose `algo=` argument fixes the path and entry points
with one path assert nothing more.  Two choices no query reports and are NOT asserted, only inferred from the width, as the path text of those cases
says: vector or guarded scalar kernels in the K x K engine (W % 4) and the 16-byte store kernel of Unpool (stride 2, even W).

A case runs once under each poison -- the guarded run first, so that an overrun shows in a band before the call ever
runs on plain allocations -- and twice clean (the engine claims run-to-run bitwise results: no atomics, every element written once; the two clean runs
are compared before anything is compared with them): all guard bands intact, all inputs bitwise unchanged, all outputs bitwise the clean run's (NaNs
canonicalised), cspn3d_check_status() quiet after a 3D call and the persistent kernel's error word 0 where the case has the workspace.  Where a
float64 statement is importable (oracle/: 2D 3 x 3 forward and backward, 3D forward and the Paddle-contract backward) the run under `ones` is also
compared with it at the tolerance of that path's own test, since the clean run is code under test as well.

Paths a small shape cannot reach through the dispatcher:
    the 12 x 3 ring    cspn2d_forward takes it from ~190 stream rows per workgroup on 256 CUs of the linear plan (tsw4_preferred): ~48 600 rows of
                       >= 256 pixels, 12.5 M pixels and 400 MB of guidance.  The case fwd2d-ring12-hook runs it at (2, 41, 260) through the hook
                       library's plan argument instead (the raw-ABI route: guarded buffers built by hand).
    cspn2d_forward_sited8   a closed experiment, compiled in experiment builds only: in the product build the case asserts the call raises before
                       anything is enqueued (and that the output it had allocated stays untouched): its three runs compare no output."""
import collections
import contextlib
import functools
import types

import numpy as np
import pytest
import torch

import cspn_amd
import memguard
from cspn_amd import _lib
from cspn_amd import functional as F
from cspn_amd import train_utils as T
from helpers import assert_close, assert_close_tight, make_inputs

DEV = "cuda"
POISONS = ("zero", "ones", "big")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


# ============================================================================================================ the detector, on the CPU
def _fake_engine(bug=None):
    """-> (namespace, call): an "engine call" in torch on CPU tensors that allocates as cspn_amd.functional does (ns.torch.empty_like, ns._workspace):
    out = a * b + 1 through a workspace.  bug: None, or one way of being wrong"""
    ns = types.SimpleNamespace(torch=torch, _workspace=lambda n, device: torch.empty(max(int(n), 1), dtype=torch.uint8, device=device))

    def call(a, b):
        out = ns.torch.empty_like(a)
        ws = ns._workspace(4 * a.numel() + 4, a.device)
        tmp = ws[:4 * a.numel()].view(torch.float32)
        extra = ws[4 * a.numel():].view(torch.float32)   # one more element, which a correct call never reads
        tmp.copy_((a * b).flatten())
        res = tmp.view(a.shape) + 1
        if bug == "stale_read":
            res = res + extra * 0.0 + extra              # (0 x keeps a NaN, + keeps a huge finite value)
        if bug == "unwritten":
            out.flatten()[:-1].copy_(res.flatten()[:-1])
        else:
            out.copy_(res)
        if bug == "past_output":
            torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel()).fill_(7.0)
        if bug == "before_workspace":
            torch.as_strided(ws, (1,), (1,), ws.storage_offset() - 1).fill_(1)
        if bug == "writes_input":
            a[0, 0] += 1.0
        return (out,)
    return ns, call


def _fake_inputs():
    gen = torch.Generator().manual_seed(1)
    return torch.randn(4, 5, generator=gen), torch.randn(4, 5, generator=gen)


def _check_poison(call, inputs, clean, poison, device_type="cuda", plane=0, modules=None, after=None, compare=True):
    """one call under `poison`: guard bands, inputs, outputs against the clean run -> (outputs, session)"""
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, call, inputs, device_type, plane, modules=modules)
        if after is not None:
            after(session)
    if compare:
        memguard.assert_same_outputs(outs, clean, "poison %r" % poison)
    return outs, session


def _detected(bug, in_guarded_run_only=False):
    """the messages of the poisons that report `bug` (a fake engine call on the CPU)"""
    ns, call = _fake_engine(bug)
    inputs = _fake_inputs()
    clean = _fake_engine(None)[1](*inputs) if in_guarded_run_only else call(*inputs)
    found = []
    for poison in POISONS:
        inputs = _fake_inputs()
        try:
            _check_poison(call, inputs, clean, poison, "cpu", modules=(ns,))
        except AssertionError as e:
            found.append(str(e))
    assert ns.torch is torch and not isinstance(ns._workspace, types.MethodType), "the patch was not undone"
    return found


def test_detector_passes_a_clean_call():
    assert _detected(None) == []
    ns, call = _fake_engine(None)
    with contextlib.ExitStack() as stack:   # and it did go through the patch: one output and one workspace were guarded
        outs, s = memguard.run_guarded(stack, "ones", call, _fake_inputs(), "cpu", modules=(ns,))
        assert len(s.guards) == 2 and len(s.workspaces) == 1 and s.workspaces[0][0].numel() == 4 * 20 + 4
        assert isinstance(ns.torch, memguard._TorchProxy) and ns.torch.float32 is torch.float32
    assert ns.torch is torch


def test_detector_reports_a_store_one_element_past_the_output():
    found = _detected("past_output", in_guarded_run_only=True)
    assert len(found) == 3 and all("guard band overwritten" in m and "first changed byte at offset 80" in m for m in found), found


def test_detector_reports_a_store_one_byte_before_the_workspace():
    found = _detected("before_workspace", in_guarded_run_only=True)
    assert len(found) == 3 and all("guard band overwritten" in m and "first changed byte at offset -1," in m for m in found), found


def test_detector_reports_an_output_element_never_written():
    found = _detected("unwritten")
    assert len(found) >= 2 and all("differs from the clean run: 1 of 20 elements, the first at flat index 19" in m for m in found), found


def test_detector_reports_a_workspace_element_read_but_never_written():
    found = _detected("stale_read")
    assert len(found) >= 2 and all("differs from the clean run" in m for m in found), found


def test_detector_reports_a_modified_input():
    found = _detected("writes_input")
    assert len(found) == 3 and all("input 0 of shape (4, 5) was modified: 1 elements, the first at flat index 0" in m for m in found), found


def test_guard_geometry_and_poison_patterns():
    t = memguard.guarded((3, 5), torch.float32, "cpu", "big", plane_bytes=100000)
    g = t._memguard
    assert g.off == 65536 and g.nbytes == 60 and g.end - g.off - g.nbytes >= 200000
    assert bool((t.view(torch.int32) == 0x7F7FFFFF).all()) and bool(torch.isfinite(t).all())
    assert int(g.buf[g.off - 1]) == 0xA5 == int(g.buf[g.off + 60])          # the bands touch the payload: it is not rounded up
    for dt in (F32, F16, BF16):
        assert bool(torch.isnan(memguard.guarded((7,), dt, "cpu", "ones")).all())
    assert memguard.back_guard_bytes(0) == 65536 == memguard.FRONT_GUARD and memguard.back_guard_bytes(40000) == 80128
    assert memguard.same_bits(torch.tensor([float("nan"), 1.0]), torch.tensor([-float("nan"), 1.0]))
    assert not memguard.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    # the arena: the same first byte for every call, the back guard behind each call's own byte count, the contents never refilled
    a = memguard.Arena(1000, "cpu")
    w1 = a.take(1000)
    w1.fill_(3)
    w2 = a.take(10)
    assert w2.data_ptr() == w1.data_ptr() and bool((w2 == 3).all())
    a.buf[memguard.FRONT_GUARD + 10] = 0
    with pytest.raises(AssertionError, match="first changed byte at offset 10, last at 10"):
        a.check()


# ============================================================================================================ the table
Case = collections.namedtuple("Case", "name covers path plane build call check_path pinned three_d ref errword")
CASES = collections.OrderedDict()


def case(name, covers, path, plane, build, call, check_path, pinned, three_d=False, ref=None, errword=None):
    """covers: the public names the case runs; path: the path it is asserted to take (check_path does the asserting, on the GPU); plane: bytes of the
    largest single plane B C [D] H W 4 (sizes the back guards); build() -> the inputs, on the GPU, made once; call(*inputs) -> a tuple of tensors;
    pinned: the test that pins the clean run of this shape and path to its float64 statement; ref(inputs, outs): the float64 statement, for `ones`;
    errword: (B, D, H, W) where the call's workspace starts with the persistent 3D kernel's, whose error word is then read"""
    assert name not in CASES, name
    covers = (covers,) if isinstance(covers, str) else tuple(covers)
    CASES[name] = Case(name, covers, path, plane, functools.lru_cache(maxsize=None)(build), call, check_path, pinned, three_d, ref, errword)


def _lib_():
    return cspn_amd.load()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t):
    """a leaf that shares t's memory (a write to it is a write to the input the snapshot watches)"""
    return t.detach().requires_grad_(True)


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _grad_close(a, ref, what):
    assert_close(_np(a).astype(np.float64), np.asarray(ref, np.float64), what, rtol=2e-4, atol_frac=5e-6)   # tests/test_backward.py, tests/test_backward3d.py


# ---- 2D, 3 x 3 ------------------------------------------------------------------------------------------------------------------------------
_RAW = {}   # case name -> the raw guidance of a 'prenorm' case (the oracle normalises it itself)


def _in2d(B, H, W, norm, sparse, seed, C=1, sparse_C=1, grad=False):
    g, h, s = make_inputs(B, H, W, seed=seed, sparse=sparse, neg=sparse)
    gen = _gen(seed + 1)
    if norm == "none":
        g = g / g.abs().sum(1, keepdim=True)
    if C > 1:
        h = torch.rand(B, C, H, W, generator=gen) * 10
        if sparse:
            s = (torch.rand(B, sparse_C, H, W, generator=gen) < 0.05).float() * (torch.rand(B, sparse_C, H, W, generator=gen) * 10 + 0.1)
    out = [g.to(DEV), h.to(DEV), None if s is None else s.to(DEV)]
    if grad:
        out.append(torch.randn(B, C, H, W, generator=gen).to(DEV))
    return tuple(out)


def _ref_fwd2d(n, norm, name=None):
    def ref(inputs, outs):
        from oracle import cspn2d_oracle
        g = _RAW[name] if norm == "prenorm" else inputs[0]
        want = cspn2d_oracle(g.cpu(), inputs[1].cpu(), None if inputs[2] is None else inputs[2].cpu(), n, "8sum" if norm == "prenorm" else norm)
        assert_close_tight(_np(outs[0]), want, "2D forward vs the oracle")   # tests/test_gpu_parity.py
    return ref


def _ref_bwd2d(n, norm, first=0):
    def ref(inputs, outs):
        from oracle.backward import cspn2d_backward_oracle
        g, h, s, go = inputs
        o, rgg, rgh = cspn2d_backward_oracle(_np(g), _np(h), _np(s), _np(go), n, norm)
        if first:
            assert_close_tight(_np(outs[0]), o, "2D forward (history) vs the oracle")
        _grad_close(outs[first], rgg, "dL/dguidance vs the oracle")
        _grad_close(outs[first + 1], rgh, "dL/dblur vs the oracle")
    return ref


def _fwd2d(name, B, H, W, n, norm, sparse, algo, path, check_path, pinned):
    def build():
        g, h, s = _in2d(B, H, W, norm, sparse, seed=B + H + W + n)
        if norm == "prenorm":
            _RAW[name] = g
            g = cspn_amd.cspn2d_normalize(g, "8sum")
        return g, h, s
    case(name, "cspn2d_forward", path, 4 * B * H * W, build, lambda g, h, s: (F.cspn2d_forward(g, h, s, n, norm, algo),), check_path, pinned,
         ref=_ref_fwd2d(n, norm, name))


def _auto2d(B, H, W, n):
    return _lib_().cspn2d_auto_algo(B, H, W, n)


def _ring(B, H, W, mask):
    return _lib.load_hooks().cspn_debug_fused2d_ring(B, H, W, int(mask))


def _is(value, want):
    assert value == want, (value, want)


_fwd2d("fwd2d-stepwise-8sum-mask", 2, 37, 53, 24, "8sum", True, "stepwise", "fold2d_kernel + step2d_kernel, one launch per step (algo='stepwise')",
       lambda: None, "test_gpu_parity.py::test_shapes (2, 37, 53, 24, '8sum', mask), every algo")
_fwd2d("fwd2d-ring8-8sum_abs", 2, 41, 260, 24, "8sum_abs", False, "auto", "the 8 x 4 assembly ring, one full first pass",
       lambda: (_is(_auto2d(2, 41, 260, 24), _lib.ALGOS["fused"]), _is(_ring(2, 41, 260, False), 8)),
       "test_backward.py (2, 41, 260, 24); the forward of this band geometry: test_gpu_parity.py::test_shapes (1, 65, 260, 24)")
_fwd2d("fwd2d-ring8-none-n36-mask", 2, 41, 260, 36, "none", True, "auto",
       "the 8 x 4 ring: a short first pass of 12 into the workspace's ping plane, then a continuation pass of 24 that reads it",
       lambda: (_is(_auto2d(2, 41, 260, 36), _lib.ALGOS["fused"]), _is(_ring(2, 41, 260, True), 8),
                _is(_lib_().cspn2d_workspace_bytes(2, 41, 260, 36) >= 4 * 2 * 41 * 260, True)),
       "test_past_4gib.py::test_2d_forward[ring8x4-continuation] (n = 36), test_gpu_parity.py::test_shapes")
_fwd2d("fwd2d-padded-compiled-8sum-mask", 2, 37, 53, 24, "8sum", True, "auto",
       "FUSED_PADDED (W % 4 != 0): planes padded to 56 columns in the workspace, the compiler-generated ring (narrower than one band)",
       lambda: (_is(_auto2d(2, 37, 53, 24), _lib.ALGOS["fused_padded"]), _is(_ring(2, 37, 56, True), 0)),
       "test_gpu_parity.py::test_shapes (2, 37, 53, 24), algos 'fused_padded' and 'auto'")
_fwd2d("fwd2d-padded-ring8-prenorm-mask", 2, 41, 302, 24, "prenorm", True, "auto",
       "FUSED_PADDED: planes padded to 304 columns with 256-byte plane tails in the workspace, the 8 x 4 assembly ring on them, norm 'prenorm'",
       lambda: (_is(_auto2d(2, 41, 302, 24), _lib.ALGOS["fused_padded"]), _is(_ring(2, 41, 304, True), 8)),
       "test_gpu_parity.py (fused_padded at W = 302 / 1218), test_past_4gib.py::test_2d_forward[padded-rows]")


def _ring12_call(g, h, s):
    """the raw-ABI route (the Python front-end cannot ask for a ring): cspn_debug_forward2d_plan with plan mode 16, buffers guarded by hand under the
    session's poison"""
    B, _, H, W = g.shape
    out = F.torch.empty_like(h)
    ws = F._workspace(_lib_().cspn2d_workspace_bytes(B, H, W, 24), g.device)
    rc = _lib.load_hooks().cspn_debug_forward2d_plan(g.data_ptr(), h.data_ptr(), s.data_ptr(), out.data_ptr(), B, H, W, 24, _lib.NORM_TYPES["8sum"], 16,
                                                     ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "cspn_debug_forward2d_plan")
    return (out,)


case("fwd2d-ring12-hook", "cspn2d_forward", "the 12 x 3 ring (tsw4_pass), asked for through the hook library's plan argument: see the module docstring", 4 * 2 * 41 * 260,
     lambda: _in2d(2, 41, 260, "8sum", True, seed=12), _ring12_call, lambda: _is(_ring(2, 41, 260, True) != 0, True),
     "test_gpu_parity.py ('fused_ring12' against the other algos), test_past_4gib.py::test_2d_forward[ring12x3]", ref=_ref_fwd2d(24, "8sum"))


def _sited8_call(g, h, s):
    if _lib.load_hooks().cspn_debug_sited8_supported(2, 41, 260, 24):
        return (cspn_amd.cspn2d_forward_sited8(cspn_amd.guidance_to_sited8(g, "8sum"), h, s, 24, "8sum"),)
    with pytest.raises(_lib.CspnError, match="experiment builds only"):
        cspn_amd.cspn2d_forward_sited8(g.view(2, 41, 130, 8, 2), h, s, 24, "8sum")
    return ()


case("fwd2d-sited8", "cspn2d_forward_sited8", "experiment builds: the sited8 loop; the product build: CspnError before any launch", 4 * 2 * 41 * 260,
     lambda: _in2d(2, 41, 260, "8sum", True, seed=8), _sited8_call, lambda: None, "test_gpu_parity.py (sited8 against cspn2d_forward, experiment builds)")

case("normalize2d-8sum", "cspn2d_normalize", "normalize2d kernel", 4 * 3 * 64 * 255, lambda: (torch.randn(3, 8, 64, 255, generator=_gen(3)).to(DEV),),
     lambda g: (cspn_amd.cspn2d_normalize(g, "8sum"),), lambda: None, "test_gpu_parity.py (gate_wb against the reference's), test_normalize_backward.py _FUZZ (3, 64, 255)")
case("normalize2d-backward-8sum_abs", ("cspn2d_normalize_backward", "cspn2d_normalize"), "normalize2d_backward kernel, directly and under autograd", 4 * 3 * 7 * 1218,
     lambda: (torch.randn(3, 8, 7, 1218, generator=_gen(4)).to(DEV), torch.randn(3, 8, 7, 1218, generator=_gen(5)).to(DEV)),
     lambda g, r: (cspn_amd.cspn2d_normalize_backward(g, r, "8sum_abs"),) + _autograd(lambda gl: cspn_amd.cspn2d_normalize(gl, "8sum_abs"), (g,), r),
     lambda: None, "test_normalize_backward.py _FUZZ (3, 7, 1218)")


def _autograd(f, leaves, grad_out, node=None, kept=None):
    """f on leaves that share the inputs' memory, backward(grad_out) -> (output, the leaves' gradients).  node: the autograd Function the output must come
    from; kept: the index of a saved tensor that must be there (the history a training-mode forward keeps)"""
    ls = [_leaf(t) for t in leaves]
    out = f(*ls)
    if node is not None:
        assert type(out.grad_fn).__name__ == node + "Backward", (type(out.grad_fn).__name__, node)
    if kept is not None:
        assert out.grad_fn.saved_tensors[kept] is not None
    out.backward(grad_out)
    return (out.detach(),) + tuple(l.grad for l in ls)


def _bwd2d(name, B, H, W, n, norm, sparse, path, asm, pinned):
    case(name, "cspn2d_backward", path, 4 * B * H * W, lambda: _in2d(B, H, W, norm, sparse, seed=B + H + W + n, grad=True),
         lambda g, h, s, go: F.cspn2d_backward(g, h, s, go, n, norm) + F.cspn2d_backward(g, h, s, go, n, norm, need_blur=False)[:1]
         + F.cspn2d_backward(g, h, s, go, n, norm, need_guidance=False)[1:],   # (both gradients, then each alone)
         lambda: _is(cspn_amd.cspn2d_history_bytes(B, H, W, n) > 0, asm), pinned,
         ref=_ref_bwd2d(n, norm))


_bwd2d("bwd2d-perstep", 2, 37, 53, 24, "8sum", True, "one launch per step: fold, n - 1 levels, transposed coefficients, n adjoint levels, final kernel", False,
       "test_backward.py::test_hip_backward_vs_oracle_and_through_autograd (2, 37, 53, 24)")
_bwd2d("bwd2d-ring-n24", 2, 41, 260, 24, "8sum", True, "the checkpointed ring path: forward and adjoint sweeps keep every fourth level, final pass of 6 segments", True,
       "test_backward.py (2, 41, 260, 24)")
_bwd2d("bwd2d-ring-n8", 1, 70, 304, 8, "8sum_abs", False, "the checkpointed ring path at n_iter 8: H_n and A_0 are checkpoint planes, 2 segments", True,
       "test_backward.py (1, 70, 304, 8)")


def _history_call(n, norm):
    def call(g, h, s, go):
        out, hist = cspn_amd.cspn2d_forward_with_history(g, h, s, n, norm)
        gg, gh = cspn_amd.cspn2d_backward_from_history(g, h, s, go, hist, n, norm)
        return out, gg, gh   # (the history itself is opaque and starts with 64 KiB nobody writes: not an output)
    return call


case("history2d-n24", ("cspn2d_forward_with_history", "cspn2d_backward_from_history"), "the level-keeping forward sweep into the history, the backward from it", 4 * 3 * 70 * 512,
     lambda: _in2d(3, 70, 512, "8sum", True, seed=21, grad=True), _history_call(24, "8sum"), lambda: _is(cspn_amd.cspn2d_history_bytes(3, 70, 512, 24) > 0, True),
     "test_backward.py::test_training_mode_history_matches_recompute_path (3, 70, 512)", ref=_ref_bwd2d(24, "8sum", first=1))
case("history2d-n12", ("cspn2d_forward_with_history", "cspn2d_backward_from_history"), "the same at n_iter 12: the result is the checkpoint H_12", 4 * 3 * 70 * 512,
     lambda: _in2d(3, 70, 512, "8sum_abs", False, seed=22, grad=True), _history_call(12, "8sum_abs"), lambda: _is(cspn_amd.cspn2d_history_bytes(3, 70, 512, 12) > 0, True),
     "test_backward.py::test_training_mode_history_matches_recompute_path (N = 12)", ref=_ref_bwd2d(12, "8sum_abs", first=1))


def _multi2d(name, B, C, H, W, n, norm, sparse_C, fast, pinned):
    def call(g, h, s, go):
        return (cspn_amd.cspn2d_forward_multi(g, h, s, n, norm),) + cspn_amd.cspn2d_backward_multi(g, h, s, go, n, norm)
    case(name, ("cspn2d_forward_multi", "cspn2d_backward_multi"),
         "one ring launch per pass over the B C image-channels, the shared mask widened in the workspace" if fast else "the per-channel loop: gathered planes in the workspace",
         4 * B * C * H * W, lambda: _in2d(B, H, W, norm, True, seed=B + C + H + W, C=C, sparse_C=sparse_C, grad=True), call,
         lambda: (_is(cspn_amd.cspn2d_multi_supported(B, C, H, W, n), fast), _is(cspn_amd.cspn2d_history_bytes(B * C, H, W, n) > 0, fast)), pinned)


_multi2d("multi2d-fast-shared-mask", 1, 2, 16, 272, 24, "8sum", 1, True, "test_multichannel.py (1, 2, 16, 272, 24), sparse 'shared'")
_multi2d("multi2d-loop-mask-per-channel", 2, 3, 11, 13, 5, "8sum_abs", 3, False, "test_multichannel.py (2, 3, 11, 13, 5), sparse 'per_channel'")


def _module2d(name, covers, make, B, H, W, n, norm, sparse, history, pinned, prenorm=False, C=1):
    def build():
        g, h, s, go = _in2d(B, H, W, "8sum" if prenorm else norm, sparse, seed=B + H + W + n + 3, C=C, grad=True)
        return (cspn_amd.cspn2d_normalize(g, "8sum") if prenorm else g), h, s, go
    case(name, covers, "forward keeping the history, backward from it" if history else "plain forward, recomputing backward", 4 * B * C * H * W, build,
         lambda g, h, s, go: _autograd(lambda gl, hl: make()(gl, hl, s), (g, h), go),
         lambda: _is((cspn_amd.cspn2d_history_bytes(B, H, W, n) if C == 1 else F.cspn2d_history_bytes_multi(B, C, H, W, n)) > 0, history), pinned)


_module2d("module-Affinity_Propagate-history", "Affinity_Propagate", lambda: cspn_amd.Affinity_Propagate(24, 3, "8sum"), 2, 41, 260, 24, "8sum", True, True,
          "test_backward.py (2, 41, 260, 24) through the module")
_module2d("module-Affinity_Propagate-plain", "Affinity_Propagate", lambda: cspn_amd.Affinity_Propagate(5, 3, "8sum_abs"), 2, 37, 53, 5, "8sum_abs", False, False,
          "test_backward.py (odd shapes through the module)")
_module2d("module-Affinity_Propagate-multi", "Affinity_Propagate", lambda: cspn_amd.Affinity_Propagate(12, 3, "8sum"), 1, 16, 272, 12, "8sum", True, True,
          "test_multichannel.py (1, 2, 16, 272, 12) through the module", C=2)
_module2d("propagate_prenorm-history", "propagate_prenorm", lambda: (lambda g, h, s: cspn_amd.propagate_prenorm(g, h, s, 12)), 2, 41, 260, 12, "prenorm", True, True,
          "test_backward.py (prenorm gradients against the oracle)", prenorm=True)
_module2d("module-Affinity_PropagateKxK-3", "Affinity_PropagateKxK", lambda: cspn_amd.Affinity_PropagateKxK(4, 3, "8sum"), 2, 41, 260, 4, "8sum", True, True,
          "test_kernel_size.py / test_kxk_norm.py (prop_kernel 3 is bitwise Affinity_Propagate); test_backward.py (2, 41, 260, 4)")


# ---- 2D, K x K ------------------------------------------------------------------------------------------------------------------------------
KXK_SHAPES = {"wide": (35, 196), "tall": (67, 70)}   # tests/test_kxk_tilegrid.py: 3 x 4 tiles with W % 4 == 0, 5 x 2 tiles with W % 4 == 2; N = 2 images


def _kxk_inputs(contract, K, H, W, dtype, seed):
    gen = _gen(seed)
    N, C = 2, 2
    g = torch.randn(N, K * K - 1, H, W, generator=gen)
    if contract == "none":
        g = g / g.abs().sum(1, keepdim=True)
    x = torch.rand(N, C, H, W, generator=gen) * (10 if contract == "norm" else 1)
    go = torch.randn(N, C, H, W, generator=gen)
    s = (torch.rand(N, C, H, W, generator=gen) < 0.05).float() * (torch.rand(N, C, H, W, generator=gen) * 10 + 0.1)
    return g.to(dtype).to(DEV), x.to(DEV), s.to(DEV), go.to(DEV)


def _kxk_call(contract, K, n):
    def call(g, x, s, go):
        if contract == "norm":
            out = F.cspn2d_forward_kxk_norm(g, x, s, K, n, "8sum_abs")
            out2, hist = F.cspn2d_forward_kxk_norm(g, x, s, K, n, "8sum_abs", return_history=True)
            gg, gx = F.cspn2d_backward_kxk_norm(g, x, s, go, K, n, "8sum_abs", hist)
            _, gx2 = F.cspn2d_backward_kxk_norm(g, x, s, go, K, n, "8sum_abs", None, need_guidance=False)   # (no dL/dguidance: the gate-gradient kernel writes dL/db only)
            return out, out2, hist, gg, gx, gx2
        fwd, bwd = (F.cspn2d_forward_kxk, F.cspn2d_backward_kxk) if contract == "none" else (F.cspn2d_forward_kxk_absnorm, F.cspn2d_backward_kxk_absnorm)
        out = fwd(g, x, K, n)
        out2, hist = fwd(g, x, K, n, return_history=True)
        gg, gx = bwd(g, x, go, K, n, hist)
        return out, out2, hist, gg, gx, bwd(g, x, go, K, n, hist, True, False)[0], bwd(g, x, go, K, n, None, False, True)[1]   # (each gradient alone)
    return call


_KXK_NAMES = {"none": ("cspn2d_forward_kxk", "cspn2d_backward_kxk"), "norm": ("cspn2d_forward_kxk_norm", "cspn2d_backward_kxk_norm"),
              "absnorm": ("cspn2d_forward_kxk_absnorm", "cspn2d_backward_kxk_absnorm")}
_KXK_PINNED = {"none": "test_kxk_tilegrid.py::test_none_op_*, test_kxk_g16.py", "norm": "test_kxk_tilegrid.py (NORM_CASES), test_kxk_g16.py",
               "absnorm": "test_kxk_absnorm.py (names 'wide', 'tall'; its 16-bit layouts)"}
for _contract in ("none", "norm", "absnorm"):
    for _K, _shape, _dt in ((5, "wide", F32), (7, "tall", F16), (7, "wide", BF16), (5, "tall", F32)):
        _H, _W = KXK_SHAPES[_shape]
        # NOT ASSERTED, inferred: no query of the library names a K x K kernel.  The vector kernels are taken where W % 4 == 0 and the tensors are aligned
        # to four elements (cspn2d_kxk.hip: forward_steps, adjoint_steps, backward_run), which a guarded tensor and a fresh allocation always are, so the
        # width decides; the path text says "inferred"
        case("kxk-%s-K%d-%s-%s" % (_contract, _K, _shape, str(_dt).split(".")[1]), _KXK_NAMES[_contract],
             "inferred from the width, not asserted: %s kernels (W %% 4 %s 0), %s; forward through the workspace's ping-pong levels, forward into the history, backward from it"
             % ("vector" if _W % 4 == 0 else "guarded scalar", "==" if _W % 4 == 0 else "!=", "float32 gates" if _dt == F32 else "16-bit gates widened where read"),
             4 * 2 * 2 * _H * _W, functools.partial(_kxk_inputs, _contract, _K, _H, _W, _dt, 10 * _K + _W), _kxk_call(_contract, _K, 3),
             lambda: None, _KXK_PINNED[_contract])

case("module-Affinity_PropagateKxK-5", "Affinity_PropagateKxK", "_CSPN2dKxKNormFunction with the history H_1 .. H_{n-1} among its saved tensors (asserted on the output's graph node), one backward call",
     4 * 2 * 2 * 35 * 196,
     functools.partial(_kxk_inputs, "norm", 5, 35, 196, F16, 77),
     lambda g, x, s, go: _autograd(lambda gl, xl: cspn_amd.Affinity_PropagateKxK(3, 5, "8sum")(gl, xl, s), (g, x), go, "_CSPN2dKxKNormFunction", 3), lambda: None,
     "test_kxk_g16.py (the module on 16-bit guidance), test_kxk_tilegrid.py 'wide'")


# ---- 3D ---------------------------------------------------------------------------------------------------------------------------------------
def _in3d(B, D, H, W, seed, raw=False, mask=False, C=1, dtype=F32, signed=True):
    gen = _gen(seed)
    g = torch.randn(B, 26, D, H, W, generator=gen) if signed else torch.rand(B, 26, D, H, W, generator=gen)
    if not raw:
        g = g / g.abs().sum(1, keepdim=True)
    h = torch.rand(B, C, D, H, W, generator=gen)
    go = torch.randn(B, C, D, H, W, generator=gen)
    s = None
    if mask:
        s = (torch.rand(B, 1, D, H, W, generator=gen) < 0.1).float() * (torch.rand(B, 1, D, H, W, generator=gen) + 0.1)
        s.view(-1)[3] = -2.5
    return g.to(dtype).to(DEV), h.to(DEV), None if s is None else s.to(DEV), go.to(DEV)


def _pers(B, D, H, W, n, C=1):
    return bool(_lib_().cspn3d_multi_supported(B, C, D, H, W, n))


def _fused_bwd3d(B, D, H, W, n, C=1):
    """whether the backward runs its fused sweeps (the level-keeping and the transposed launch of the persistent kernel) at this shape, asked of the library:
    the 16-bit workspace query is larger than the float32 one exactly where cspn3d_backward.hip's fused3d_shape holds (the widened copy of the gates the
    transposed sweep reads; tests/test_3d_g16.py pins that).  The call's own part of the condition, 16-byte aligned tensors, holds for every guarded tensor
    and every fresh allocation"""
    if C == 1:
        return _lib.symbol("cspn3d_backward_g16_workspace_bytes")(B, D, H, W, n) > _lib.symbol("cspn3d_backward_workspace_bytes")(B, D, H, W, n)
    return _lib.symbol("cspn3d_backward_multi_g16_workspace_bytes")(B, C, D, H, W, n) > _lib.symbol("cspn3d_backward_multi_workspace_bytes")(B, C, D, H, W, n)


def _ref_fwd3d(n, norm):
    def ref(inputs, outs):
        from oracle import cspn3d_oracle
        g, h, s, _ = inputs
        assert_close(_np(outs[0]), cspn3d_oracle(g.float().cpu(), h.cpu(), None if s is None else s.cpu(), n, norm), "3D forward vs the oracle")   # tests/test_gpu_parity.py
    return ref


def _ref_bwd3d(n):
    def ref(inputs, outs):
        from oracle.backward import cspn3d_backward_oracle
        g, h, _, go = inputs
        dG, dF = cspn3d_backward_oracle(_np(g), _np(h), _np(go), n)
        _grad_close(outs[0], dG, "dL/dgate vs the oracle")
        _grad_close(outs[1], dF, "dL/dfeat vs the oracle")
    return ref


def _fwd3d(name, shape, n, norm, mask, algo, path, check_path, pinned, dtype=F32, errword=False, entry="cspn3d_forward"):
    B, D, H, W = shape
    f = getattr(F, entry)
    case(name, entry, path, 4 * B * D * H * W, lambda: _in3d(B, D, H, W, sum(shape) + n, raw=norm != "none", mask=mask, dtype=dtype, signed=norm != "8sum_abs"),
         lambda g, h, s, go: (f(g, h, s, n, norm, algo),), check_path, pinned, three_d=True, ref=_ref_fwd3d(n, norm), errword=shape if errword else None)


_fwd3d("fwd3d-perstep-direct", (1, 4, 6, 16), 3, "none", False, "stepwise", "step3d_direct_kernel (W % 4 == 0, quads), one launch per step, ping-pong volumes in the workspace",
       lambda: None, "test_gpu_parity.py::test_3d_parity_vs_oracle, test_3d_g16.py STEPWISE shapes")
_fwd3d("fwd3d-perstep-scalar-none", (2, 4, 5, 7), 3, "none", False, "auto", "W % 4 != 0: fold3d_kernel into 27 planes, then step3d_kernel voxel by voxel",
       lambda: _is(_pers(2, 4, 5, 7, 3), False), "test_gpu_parity.py::test_3d_parity_vs_oracle (2, 4, 5, 7)")
_fwd3d("fwd3d-perstep-folded-8sum-mask", (1, 2, 5, 10), 3, "8sum", True, "stepwise", "the folded modes per step: fold3d_kernel (normalise, site, pin), step3d_kernel",
       lambda: None, "test_gpu_parity.py::test_3d_parity_vs_oracle (1, 2, 5, 10)")
_fwd3d("fwd3d-perstep-folded-8sum_abs-mask", (1, 4, 6, 16), 3, "8sum_abs", True, "stepwise", "the folded modes per step at W % 4 == 0", lambda: None,
       "test_gpu_parity.py::test_3d_parity_vs_oracle (1, 4, 6, 16)")
_fwd3d("fwd3d-persistent-one-tile", (1, 8, 8, 64), 12, "none", False, "persistent", "the persistent kernel, one tile, 12 steps", lambda: _is(_pers(1, 8, 8, 64, 12), True),
       "test_gpu_parity.py::test_3d_persistent_vs_stepwise_and_oracle (1, 8, 8, 64)", errword=True)
_fwd3d("fwd3d-persistent-tiles", (2, 20, 30, 200), 12, "none", False, "auto", "the persistent kernel (the dispatcher's choice): several tiles in z, y and x, chunks",
       lambda: _is(_pers(2, 20, 30, 200, 12), True), "test_backward3d.py (2, 20, 30, 200, 12), test_gpu_parity.py persistent shapes", errword=True)
_fwd3d("fwd3d-persistent-folded-mask", (1, 8, 8, 64), 12, "8sum_abs", True, "persistent", "fold3d_kernel, then the persistent kernel on the 27 folded planes (c' in LDS)",
       lambda: _is(_pers(1, 8, 8, 64, 12), True), "test_gpu_parity.py (folded modes, algo='persistent'), test_backward3d_norm.py FUSED_CASES (1, 8, 8, 64)")
_fwd3d("fwd3d-persistent-f16", (1, 8, 8, 64), 12, "none", False, "persistent", "the persistent kernel's float16 instance (cspn3d_forward_g16_algo)",
       lambda: _is(_pers(1, 8, 8, 64, 12), True), "test_3d_g16.py::test_none_forward_is_bitwise_the_float32_engine", dtype=F16, errword=True)
_fwd3d("fwd3d-norm-bf16-mask", (1, 4, 6, 16), 3, "8sum_abs", True, "stepwise", "cspn3d_forward_norm_g16: fold3d_kernel<bf16>, per-step", lambda: None,
       "test_backward3d_norm_g16.py (the forward's bitwise twin)", dtype=BF16, entry="cspn3d_forward_norm")

case("fwd3d-multi", "cspn3d_forward_multi", "the persistent kernel's MULTI instance: C = 3 channels on shared gates, one launch", 4 * 2 * 3 * 20 * 30 * 200,
     lambda: _in3d(2, 20, 30, 200, 5, C=3), lambda g, h, s, go: (F.cspn3d_forward_multi(g, h, 12),), lambda: _is(_pers(2, 20, 30, 200, 12, 3), True),
     "test_gpu_parity.py::test_3d_shared_gates_multi_channel_equals_per_channel_loop", three_d=True, errword=(2, 20, 30, 200))
case("fwd3d-absnorm-persistent", "cspn3d_forward_absnorm", "cspn3d_forward_absnorm_f32: the NRM instance normalises the resident gates", 4 * 2 * 6 * 10 * 64,
     lambda: _in3d(2, 6, 10, 64, 6, raw=True), lambda g, h, s, go: (F.cspn3d_forward_absnorm(g, h, 12, "persistent"),), lambda: _is(_pers(2, 6, 10, 64, 12), True),
     "test_absnorm.py (2, 6, 10, 64, 12)", three_d=True, errword=(2, 6, 10, 64))
case("fwd3d-absnorm-perstep", "cspn3d_forward_absnorm", "cspn3d_forward_absnorm_f32 unfused: the normaliser into the workspace, then the folding per-step path (W % 4 != 0)",
     4 * 2 * 3 * 5 * 7, lambda: _in3d(2, 3, 5, 7, 7, raw=True), lambda g, h, s, go: (F.cspn3d_forward_absnorm(g, h, 3),), lambda: _is(_pers(2, 3, 5, 7, 3), False),
     "test_absnorm.py (2, 3, 5, 7, 3)", three_d=True)


def _bwd3d(name, shape, n, fused, path, pinned, C=1, dtype=F32, ref=True):
    B, D, H, W = shape
    f = F.cspn3d_backward if C == 1 else F.cspn3d_backward_multi
    case(name, f.__name__, path, 4 * B * C * D * H * W, lambda: _in3d(B, D, H, W, sum(shape) + n + C, C=C, dtype=dtype),
         lambda g, h, s, go: f(g, h, go, n) + f(g, h, go, n, need_feat=False)[:1] + f(g, h, go, n, need_gate=False)[1:],   # (without grad_feat, A_0 lives in the workspace)
         lambda: _is(_fused_bwd3d(B, D, H, W, n, C), fused), pinned, three_d=True, ref=_ref_bwd3d(n) if ref and C == 1 else None)


_bwd3d("bwd3d-fused-one-tile", (1, 8, 8, 64), 3, True, "fused sweeps: level-keeping forward launch, transposed launch, gate-gradient pass", "test_backward3d.py (1, 8, 8, 64, 3)")
_bwd3d("bwd3d-fused-tiles", (2, 20, 30, 200), 12, True, "fused sweeps over several tiles and chunks", "test_backward3d.py (2, 20, 30, 200, 12)")
_bwd3d("bwd3d-perstep-vector", (1, 4, 6, 16), 2, False, "one launch per step (n < 3): step3d_direct, adjoint3d_kernel<4>, gate_grad3d_kernel<4>", "test_backward3d.py (n below the fused sweeps)")
_bwd3d("bwd3d-perstep-scalar", (2, 4, 5, 7), 3, False, "one launch per step, W % 4 != 0: the one-voxel kernels", "test_backward3d.py (2, 4, 5, 8, 1) / (1, 3, 6, 7, 4)")
_bwd3d("bwd3d-fused-f16", (1, 8, 8, 64), 3, True, "fused sweeps on float16 gates: the widened float32 copy behind the workspace for the transposed sweep",
       "test_3d_g16.py (backward, fused)", dtype=F16, ref=False)
_bwd3d("bwd3d-multi-fused", (1, 8, 8, 64), 3, True, "fused sweeps, C = 2: the MULTI instances", "test_backward3d.py (multi-channel against the oracle per channel)", C=2)
_bwd3d("bwd3d-multi-perstep", (2, 4, 5, 7), 3, False, "one launch per step and channel", "test_backward3d.py (multi-channel, odd shapes)", C=2)


def _bwd3d_norm(name, shape, n, norm, dtype, path, pinned, fused):
    """fused: the adjoint sweep runs in the persistent kernel's transposed instance (backward3d_norm_fused: the conditions of cspn3d_backward's fused sweeps)"""
    B, D, H, W = shape
    case(name, "cspn3d_backward_norm", path, 4 * B * D * H * W, lambda: _in3d(B, D, H, W, sum(shape) + n, raw=True, mask=True, dtype=dtype, signed=False),
         lambda g, h, s, go: F.cspn3d_backward_norm(g, h, s, go, n, norm), lambda: _is(_fused_bwd3d(B, D, H, W, n), fused), pinned, three_d=True)


_bwd3d_norm("bwd3d-norm-8sum_abs-mask", (1, 8, 8, 64), 3, "8sum_abs", F32,
            "cspn3d_backward_norm_f32: the fold recomputed, the adjoint sweep in the persistent kernel's transposed instance",
            "test_backward3d_norm.py FUSED_CASES (1, 8, 8, 64), 3", True)
_bwd3d_norm("bwd3d-norm-8sum_abs-mask-bf16", (1, 8, 8, 64), 3, "8sum_abs", BF16, "cspn3d_backward_norm_g16", "test_backward3d_norm_g16.py (1, 8, 8, 64)", True)
_bwd3d_norm("bwd3d-norm-8sum-mask-odd", (2, 4, 5, 7), 1, "8sum", F32, "cspn3d_backward_norm_f32, W % 4 != 0: the scalar kernels", "test_backward3d_norm.py CASES (2, 4, 5, 7), 1", False)

case("module-Affinity_Propagate3d", "Affinity_Propagate3d", "_CSPN3dNormFunction: cspn3d_forward_norm and cspn3d_backward_norm, both per step (W = 16 is narrower than a tile)",
     4 * 1 * 4 * 6 * 16,
     lambda: _in3d(1, 4, 6, 16, 31, raw=True, mask=True, signed=False),
     lambda g, h, s, go: _autograd(lambda gl, hl: cspn_amd.Affinity_Propagate3d(3)(gl, hl, s), (g, h), go, "_CSPN3dNormFunction"),
     lambda: (_is(_pers(1, 4, 6, 16, 3), False), _is(_fused_bwd3d(1, 4, 6, 16, 3), False)),
     "test_backward3d_norm.py (through the module)", three_d=True)
case("module-Affinity_Propagate3d-bf16", "Affinity_Propagate3d", "the same on bfloat16 guidance, W % 4 != 0: per step, the one-voxel kernels", 4 * 2 * 4 * 5 * 7,
     lambda: _in3d(2, 4, 5, 7, 32, raw=True, mask=True, signed=False, dtype=BF16),
     lambda g, h, s, go: _autograd(lambda gl, hl: cspn_amd.Affinity_Propagate3d(2, 3, "8sum")(gl, hl, s), (g, h), go, "_CSPN3dNormFunction"),
     lambda: (_is(_pers(2, 4, 5, 7, 2), False), _is(_fused_bwd3d(2, 4, 5, 7, 2), False)),
     "test_backward3d_norm_g16.py (through the module)", three_d=True)


# ---- the demo module, affinity_propagate, gate_absnorm ----------------------------------------------------------------------------------------
def _cspn_inputs(dim, C, S, K, dtype, seed):
    gen = _gen(seed)
    N = 2 if dim == 2 else 1
    guide = torch.randn(N, C * (K ** dim - 1), *S, generator=gen)
    return guide.to(dtype).to(DEV), torch.rand(N, C, *S, generator=gen).to(DEV), torch.randn(N, C, *S, generator=gen).to(DEV)


def _cspn_case(name, dim, C, S, K, n, dtype, path, check_path, pinned):
    numel = 4 * (2 if dim == 2 else 1) * C * int(np.prod(S))
    case(name, ("CSPN", "absnorm_propagate"), path, numel, functools.partial(_cspn_inputs, dim, C, S, K, dtype, n + C + sum(S)),
         lambda guide, x, go: _autograd(lambda gl, xl: cspn_amd.CSPN(dim, C, K, n)(gl, xl), (guide, x), go, "_AbsnormPropagateFunction"), check_path, pinned, three_d=dim == 3)


_cspn_case("module-CSPN-2d-3x3", 2, 2, (16, 264), 3, 8, F32,
           "gate_absnorm, the 8 x 4 ring forward on 'none' over the folded batch of 4, the checkpointed ring backward, gate_absnorm_backward",
           lambda: (_is(_auto2d(4, 16, 264, 8), _lib.ALGOS["fused"]), _is(_ring(4, 16, 264, False), 8), _is(cspn_amd.cspn2d_history_bytes(4, 16, 264, 8) > 0, True)),
           "test_absnorm.py (2, 2, (16, 264), 8)")
_cspn_case("module-CSPN-2d-5x5-bf16", 2, 2, (18, 259), 5, 3, BF16,
           "cspn2d_forward_kxk_absnorm_g16 keeping the levels, cspn2d_backward_kxk_absnorm_g16 (the K x K engine's one host path; its scalar kernels at this odd width: inferred)",
           lambda: None,
           "test_kxk_absnorm.py (the module, 16-bit guides; 'strip')")
_cspn_case("module-CSPN-3d", 3, 2, (3, 5, 12), 3, 3, F32,
           "cspn3d_forward_absnorm unfused (W = 12 is narrower than a tile: the normaliser, then one launch per step), then gate_absnorm + cspn3d_backward per step + the "
           "normaliser's backward on the folded batch of 2", lambda: (_is(_pers(2, 3, 5, 12, 3), False), _is(_fused_bwd3d(2, 3, 5, 12, 3), False)),
           "test_absnorm.py (3, 2, (3, 5, 12), 3)")
_cspn_case("module-CSPN-3d-f16-persistent", 3, 1, (4, 6, 64), 3, 4, F16, "the same on a float16 guide where the persistent kernel and the backward's fused sweeps run",
           lambda: (_is(_pers(1, 4, 6, 64, 4), True), _is(_fused_bwd3d(1, 4, 6, 64, 4), True)),
           "test_absnorm.py (3, 1, (4, 6, 64), 4), test_3d_g16.py (the module)")


def _ap_case(name, dim, C, S, K, n, grad, path, check_path, pinned, node=None):
    def build():
        gen = _gen(n + C + sum(S) + K)
        g = torch.randn(2, K ** dim - 1, *S, generator=gen)
        g = g / g.abs().sum(1, keepdim=True)
        return g.to(DEV), torch.rand(2, C, *S, generator=gen).to(DEV), torch.randn(2, C, *S, generator=gen).to(DEV)

    def call(g, x, go):
        if grad:
            return _autograd(lambda xl, gl: cspn_amd.affinity_propagate(xl, gl, K, n), (x, g), go, node)
        with torch.no_grad():
            return (cspn_amd.affinity_propagate(x, g, K, n),)
    case(name, "affinity_propagate", path, 4 * 2 * C * int(np.prod(S)), build, call, check_path, pinned, three_d=dim == 3)


_ap_case("affinity_propagate-2d-C1-grad", 2, 1, (37, 53), 3, 3, True, "_AffinityPropagateFunction: cspn2d_forward on 'none' (FUSED_PADDED at W = 53), the per-step cspn2d_backward",
         lambda: (_is(_auto2d(2, 37, 53, 3), _lib.ALGOS["fused_padded"]), _is(cspn_amd.cspn2d_history_bytes(2, 37, 53, 3), 0)), "test_backward.py, test_model.py",
         node="_AffinityPropagateFunction")
_ap_case("affinity_propagate-2d-C2", 2, 2, (16, 272), 3, 24, False, "cspn2d_forward_multi", lambda: _is(cspn_amd.cspn2d_multi_supported(2, 2, 16, 272, 24), True), "test_multichannel.py")
_ap_case("affinity_propagate-2d-5x5-grad", 2, 2, (35, 196), 5, 3, True, "_AffinityPropagateKxKFunction (asserted on the output's graph node; the K x K engine's one host path)", lambda: None,
         "test_kernel_size.py, test_kxk_tilegrid.py 'wide'", node="_AffinityPropagateKxKFunction")
_ap_case("affinity_propagate-3d-C3", 3, 3, (8, 8, 64), 3, 4, False, "cspn3d_forward_multi", lambda: _is(_pers(2, 8, 8, 64, 4, 3), True), "test_gpu_parity.py (affinity_propagate, C > 1)")
_ap_case("affinity_propagate-3d-C2-grad", 3, 2, (4, 5, 7), 3, 3, True, "_AffinityPropagateFunction in 3D: the per-channel forward loop, cspn3d_backward_multi",
         lambda: (_is(_pers(2, 4, 5, 7, 3, 2), False), _is(_fused_bwd3d(2, 4, 5, 7, 3, 2), False)), "test_backward3d.py (through affinity_propagate)",
         node="_AffinityPropagateFunction")

for _K, _shape in ((26, (2, 52, 3, 5, 7)), (8, (3, 16, 7, 9)), (24, (2, 24, 9, 13))):
    case("gate_absnorm-K%d" % _K, "gate_absnorm", "cspn_gate_absnorm_f32 and, under autograd, cspn_gate_absnorm_backward_f32", 4 * int(np.prod(_shape)),
         functools.partial(lambda shape: (torch.randn(*shape, generator=_gen(shape[1])).to(DEV), torch.randn(*shape, generator=_gen(shape[1] + 1)).to(DEV)), _shape),
         functools.partial(lambda K, g, r: (cspn_amd.gate_absnorm(g, K),) + _autograd(lambda gl: cspn_amd.gate_absnorm(gl, K), (g,), r)
                           + (F.gate_absnorm_backward(g, r, K),), _K),
         lambda: None, "test_absnorm.py (K = 26 / 8 shapes), test_kxk_absnorm.py (K = 24)", three_d=False)


# ---- the heads ----------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPE = (3, 64, 40, 125, 79, 249)   # tests/test_head.py, tests/test_head_kxk.py: cropped (H < 2 h), odd W


def _head_inputs(P, dtype, seed):
    B, C, h, w, H, W = HEAD_SHAPE
    gen = _gen(seed)
    x = torch.randn(B, C, h, w, generator=gen).to(DEV).to(dtype)
    wg = (torch.randn(P, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)).to(DEV)
    wb = (torch.randn(1, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)).to(DEV)
    gg = torch.randn(B, P, H, W, generator=gen).to(DEV).to(dtype if (P != 8 and dtype != F32) else F32)
    gb = torch.randn(B, 1, H, W, generator=gen).to(DEV)
    return x, wg, wb, gg, gb


def _head_case(P, dtype, key, pinned):
    gd = F32 if (P == 8 and dtype != F32) else None
    H, W = HEAD_SHAPE[4:]

    def call(x, wg, wb, gg, gb):
        outs = T.guidance_heads(x, wg, wb, H, W, guidance_dtype=gd) + T.guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=gd)
        if key == "f32":   # the normalisation fused behind the conv (grad off)
            with torch.no_grad():
                outs = outs + T.guidance_heads(x, wg, wb, H, W, norm_type="8sum")
        return outs
    case("heads-%d-%s" % (P, str(dtype).split(".")[1]), ("guidance_heads", "guidance_heads_backward"),
         "_HEAD_PATHS[%r]: %s, forward and backward, output cropped to %d x %d" % (key, T._HEAD_PATHS[key].fwd, H, W), 4 * HEAD_SHAPE[0] * P * H * W,
         functools.partial(_head_inputs, P, dtype, P + (dtype == BF16)), call,
         lambda: _is(T._head_path(torch.empty(1, 1, 1, 1, dtype=dtype), torch.empty(P, 1, 3, 3), None, P, gd) is T._HEAD_PATHS[key], True), pinned)


_head_case(8, F32, "f32", "test_head.py (3, 40, 125, 79, 249), test_head_host_path.py")
_head_case(24, F32, "kxk_f32", "test_head_kxk.py (3, 40, 125, 79, 249), K = 5")
_head_case(48, F32, "kxk_f32", "test_head_kxk.py (3, 40, 125, 79, 249), K = 7")
_head_case(8, F16, "g16", "test_head_g16.py (cropped shapes), test_head_host_path.py D")
_head_case(24, BF16, "kxk_g16", "test_head_kxk_g16.py, test_head_host_path.py C")
_head_case(48, F16, "kxk_g16", "test_head_kxk_g16.py")


def _heads_module_path(P, dtype, key):
    """the path GuidanceHeads.forward selects for this x: guidance_dtype float32 for a 16-bit x on the 8-plane head"""
    gd = F32 if (P == 8 and dtype != F32) else None
    return lambda: _is(T._head_path(torch.empty(1, 1, 1, 1, dtype=dtype), torch.empty(P, 1, 3, 3), None, P, gd) is T._HEAD_PATHS[key], True)


def _heads_module_call(K, H, W):
    def call(x, wg, wb, gg, gb):
        m = T.GuidanceHeads(x.shape[1], K, H, W)
        m.weight_guidance, m.weight_blur = torch.nn.Parameter(wg), torch.nn.Parameter(wb)   # (the inputs' own memory)
        xl = _leaf(x)
        g, b = m(xl)
        assert type(g.grad_fn).__name__ == "_GuidanceHeadsFunctionBackward" and b.grad_fn is g.grad_fn
        ((g.float() * gg.float()).sum() + (b * gb).sum()).backward()
        return g.detach(), b.detach(), xl.grad, m.weight_guidance.grad, m.weight_blur.grad
    return call


case("module-GuidanceHeads-3-f32", "GuidanceHeads", "_GuidanceHeadsFunction on _HEAD_PATHS['f32']", 4 * 3 * 8 * 79 * 249, functools.partial(_head_inputs, 8, F32, 90),
     _heads_module_call(3, 79, 249), _heads_module_path(8, F32, "f32"), "test_head_host_path.py (autograd step, path A)")
case("module-GuidanceHeads-5-bf16", "GuidanceHeads", "_GuidanceHeadsFunction on _HEAD_PATHS['kxk_g16']", 4 * 3 * 24 * 79 * 249, functools.partial(_head_inputs, 24, BF16, 91),
     _heads_module_call(5, 79, 249), _heads_module_path(24, BF16, "kxk_g16"), "test_head_host_path.py (autograd step, path C)")
case("module-GuidanceHeads-3-f16", "GuidanceHeads", "_GuidanceHeadsFunction on _HEAD_PATHS['g16'] (guidance_dtype float32)", 4 * 3 * 8 * 79 * 249,
     functools.partial(_head_inputs, 8, F16, 92), _heads_module_call(3, 79, 249), _heads_module_path(8, F16, "g16"), "test_head_host_path.py (autograd step, path D)")


# ---- the steps next to the path -----------------------------------------------------------------------------------------------------------------
def _depth_pair(shape, seed):
    gen = _gen(seed)
    gt = torch.rand(*shape, generator=gen) * 10
    gt[torch.rand(*shape, generator=gen) < 0.3] = 0.0
    return gt.to(DEV), (torch.rand(*shape, generator=gen) * 10 + 0.05).to(DEV)


case("evaluate_error", "evaluate_error", "metrics_partial_kernel into the workspace's per-block sums, metrics_final_kernel", 4 * 2 * 37 * 53, lambda: _depth_pair((2, 1, 37, 53), 40),
     lambda gt, pred: (torch.tensor(list(T.evaluate_error(gt, pred).values()), dtype=torch.float64),), lambda: None, "test_train_utils.py ((2, 1, 37, 53), 0.3)")
case("Wighted_L1_Loss", "Wighted_L1_Loss", "_L1: the metrics kernels forward, l1_backward_kernel", 4 * 2 * 37 * 53, lambda: _depth_pair((2, 1, 37, 53), 41),
     lambda gt, pred: _autograd(lambda p: T.Wighted_L1_Loss()(p, gt), (pred,), torch.tensor(1.5, device=DEV)), lambda: None, "test_train_utils.py (the loss and its gradient)")


def _unpool_case(name, shape, stride, vec, pinned):
    N, C, H, W = shape
    # NOT ASSERTED, inferred: no query names the kernel.  cspn_aux.hip cspn_unpool_f32 takes the 16-byte store kernel where stride == 2, W is even, x is
    # 8-byte and out 16-byte aligned (guarded tensors and fresh allocations are)
    assert vec == (stride == 2 and W % 2 == 0)
    case(name, "Unpool", "inferred from stride and width, not asserted: " + ("unpool2_kernel (16-byte stores)" if vec else "unpool_kernel (one element per thread)"),
         4 * N * C * H * W * stride * stride,
         lambda: (torch.randn(*shape, generator=_gen(H + W)).to(DEV), torch.randn(N, C, H * stride, W * stride, generator=_gen(H)).to(DEV)),
         lambda x, go: _autograd(lambda xl: T.Unpool(C, stride)(xl), (x,), go, "_Unpool"), lambda: None, pinned)


_unpool_case("Unpool-stride2-even", (1, 64, 57, 76), 2, True, "test_train_utils.py (1, 64, 57, 76, 2)")
_unpool_case("Unpool-stride2-odd", (2, 3, 5, 7), 2, False, "test_train_utils.py (2, 3, 5, 7, 2)")
_unpool_case("Unpool-stride3", (1, 1, 4, 4), 3, False, "test_train_utils.py (1, 1, 4, 4, 3)")

for _mode in ("nyu", "kitti"):
    case("createSparseDepthImage-" + _mode, "createSparseDepthImage",
         "sparse_sample_kernel, hw %% 4 != 0%s" % (" behind count_valid_kernel (per-image counts in the workspace)" if _mode == "kitti" else ""),
         4 * 2 * 37 * 53, lambda: (_depth_pair((2, 1, 37, 53), 42)[0],), functools.partial(lambda mode, d: (T.createSparseDepthImage(d, 500, mode, seed=7),), _mode),
         lambda: _is((37 * 53) % 4 != 0, True), "test_train_utils.py (createSparseDepthImage, (2, 1, 37, 53))")


# ---- the variants the issue lists, by the case that runs each -----------------------------------------------------------------------------------
VARIANTS = {
    "2D fwd stepwise": "fwd2d-stepwise-8sum-mask", "2D fwd 8 x 4 ring": "fwd2d-ring8-8sum_abs", "2D fwd 12 x 3 ring": "fwd2d-ring12-hook",
    "2D fwd FUSED_PADDED": "fwd2d-padded-ring8-prenorm-mask", "2D fwd FUSED_PADDED narrow": "fwd2d-padded-compiled-8sum-mask",
    "2D fwd norm 8sum": "fwd2d-stepwise-8sum-mask", "2D fwd norm 8sum_abs": "fwd2d-ring8-8sum_abs", "2D fwd norm none": "fwd2d-ring8-none-n36-mask",
    "2D fwd norm prenorm": "fwd2d-padded-ring8-prenorm-mask", "2D fwd without sparse": "fwd2d-ring8-8sum_abs", "2D fwd with sparse": "fwd2d-ring8-none-n36-mask",
    "2D bwd per step": "bwd2d-perstep", "2D bwd ring n 24": "bwd2d-ring-n24", "2D bwd ring n 4..20": "bwd2d-ring-n8", "2D bwd from history": "history2d-n24",
    "2D multi fwd+bwd": "multi2d-fast-shared-mask", "2D multi loop": "multi2d-loop-mask-per-channel",
    "3D fwd per-step vector": "fwd3d-perstep-direct", "3D fwd scalar": "fwd3d-perstep-scalar-none", "3D fwd folded mask": "fwd3d-perstep-folded-8sum_abs-mask",
    "3D persistent plain": "fwd3d-persistent-tiles", "3D persistent folded": "fwd3d-persistent-folded-mask", "3D persistent multi": "fwd3d-multi",
    "3D persistent absnorm": "fwd3d-absnorm-persistent", "3D persistent 16-bit": "fwd3d-persistent-f16",
    "3D bwd fused": "bwd3d-fused-tiles", "3D bwd per step": "bwd3d-perstep-scalar", "3D bwd multi fused": "bwd3d-multi-fused", "3D bwd multi per step": "bwd3d-multi-perstep",
    "3D bwd norm 8sum_abs mask": "bwd3d-norm-8sum_abs-mask", "3D bwd norm g16": "bwd3d-norm-8sum_abs-mask-bf16",
    "heads 8": "heads-8-float32", "heads 24": "heads-24-float32", "heads 48": "heads-48-float32", "heads 16-bit": "heads-24-bfloat16", "heads 8 16-bit": "heads-8-float16",
    "gate_absnorm": "gate_absnorm-K26", "normalize": "normalize2d-8sum", "normalize backward": "normalize2d-backward-8sum_abs",
    "Unpool 16-byte stores": "Unpool-stride2-even", "Unpool scalar": "Unpool-stride3", "createSparseDepthImage": "createSparseDepthImage-kitti",
}
for _c in ("none", "norm", "absnorm"):
    VARIANTS.update({"kxk %s K5 f32 vector" % _c: "kxk-%s-K5-wide-float32" % _c, "kxk %s K7 16-bit scalar" % _c: "kxk-%s-K7-tall-float16" % _c,
                     "kxk %s K7 16-bit vector" % _c: "kxk-%s-K7-wide-bfloat16" % _c, "kxk %s K5 f32 scalar" % _c: "kxk-%s-K5-tall-float32" % _c})
NOT_BITWISE = {}   # case name -> the reason, for a path that turned out not to be run-to-run bitwise (then compared with its float64 statement instead): none


def test_the_table_is_complete():
    import inspect
    required = (set(cspn_amd.__all__) - {"build", "load", "CspnError", "cspn3d_check_status"}) | {
        "cspn2d_forward_with_history", "cspn2d_backward_from_history", "cspn2d_forward_sited8", "evaluate_error", "Wighted_L1_Loss", "Unpool", "createSparseDepthImage"}
    covered = {n for c in CASES.values() for n in c.covers}
    assert required <= covered, sorted(required - covered)
    for n in covered:
        assert any(hasattr(m, n) for m in (cspn_amd, F, T)), n
    for what, name in VARIANTS.items():
        assert name in CASES, (what, name)
    for c in CASES.values():
        assert c.path and c.pinned and c.plane > 0, c.name
    for m in ("Affinity_Propagate", "Affinity_PropagateKxK", "Affinity_Propagate3d", "CSPN", "propagate_prenorm", "GuidanceHeads", "Wighted_L1_Loss", "Unpool"):
        assert any(m in c.covers and (c.name.startswith("module-") or m in c.name) for c in CASES.values()), m
    # cspn_amd/cspn.py allocates nothing itself (if it ever does, memguard.patched has to cover it); the two patched modules go through the names patched
    from cspn_amd import cspn
    src = inspect.getsource(cspn)
    for alloc in ("torch.empty", "torch.zeros", "torch.ones", ".new_empty", ".new_zeros", "_workspace"):
        assert alloc not in src, alloc
    assert "torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)" in inspect.getsource(F._workspace)
    assert T._launch is F._launch and set(NOT_BITWISE) <= set(CASES)


# ============================================================================================================ GPU: the cases under the poisons
_CLEAN = {}


def _clean(c):
    """the clean (unpatched) run, made once per case and shared; made twice first: the engine's claim of run-to-run bitwise results"""
    if c.name not in _CLEAN:
        inputs = c.build()
        a = c.call(*inputs)
        b = c.call(*inputs)
        if c.three_d:
            F.cspn3d_check_status()
        torch.cuda.synchronize()
        if c.name not in NOT_BITWISE:
            memguard.assert_same_outputs(b, a, "second clean run")
        _CLEAN[c.name] = a
    return _CLEAN[c.name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("poison", POISONS)      # (the decorator nearest the function is the outer loop: every case under 'zero' first, then 'ones', then 'big')
def test_case_under_poison(name, poison):
    """the guarded run comes first: an overrun is then reported from inside a guard band before the call ever runs on plain allocations"""
    c = CASES[name]
    c.check_path()
    inputs = c.build()

    def after(session):
        if c.three_d:
            F.cspn3d_check_status()   # raises CspnError if a persistent launch gave up
        if c.errword is not None:
            assert session.workspaces, "the case has no workspace"
            for ws, _ in session.workspaces:
                assert _lib.load_hooks().cspn_debug_3d_persistent_error(ws.data_ptr(), *c.errword) == 0
    bitwise = c.name not in NOT_BITWISE
    assert bitwise or c.ref is not None, "a path marked not bitwise is compared with its float64 statement instead: it needs one"
    outs, _ = _check_poison(c.call, inputs, None, poison, "cuda", c.plane, after=after, compare=False)
    if bitwise:
        memguard.assert_same_outputs(outs, _clean(c), "poison %r" % poison)
    if c.ref is not None and (poison == "ones" or not bitwise):
        c.ref(inputs, outs)


# ============================================================================================================ GPU: stale workspaces, one arena
def _run_sequence(steps, plane, three_d=False):
    """steps: (label, call, inputs[, (B, D, H, W) where the call's workspace starts with the persistent 3D kernel's: its error word is then read in the arena]).
    Every call once between guard bands (which also tells the workspace sizes asked for) and once on clean memory, then the
    whole sequence through ONE arena sized to the largest request and never refilled: guards, inputs, and every result bitwise the clean one"""
    clean, sizes = [], []
    with contextlib.ExitStack() as stack:   # guarded first (an overrun shows in a band before anything runs on plain allocations); this pass has the sizes
        session = memguard.patched(stack, "zero", plane_bytes=plane)
        for label, call, inputs in (s[:3] for s in steps):
            call(*inputs)
            session.check()
        sizes = [n for _, n in session.workspaces]
    for label, call, inputs in (s[:3] for s in steps):
        clean.append(call(*inputs))
    if three_d:
        F.cspn3d_check_status()
    torch.cuda.synchronize()
    assert sizes and max(sizes) > 0
    arena = memguard.Arena(max(sizes), DEV, plane)
    with contextlib.ExitStack() as stack:
        session = memguard.patched(stack, "stale", arena=arena, plane_bytes=plane)
        for i, (label, call, inputs, *errword) in enumerate(steps):
            snap = memguard.snapshot(*inputs)
            taken = arena.taken
            outs = call(*inputs)
            session.check()
            snap.assert_unchanged()
            if three_d:
                F.cspn3d_check_status()
            if errword:
                assert arena.taken == taken + 1, "the step took %d workspaces" % (arena.taken - taken)
                assert _lib.load_hooks().cspn_debug_3d_persistent_error(arena.current.payload().data_ptr(), *errword[0]) == 0, label
            memguard.assert_same_outputs(outs, clean[i], "step %d (%s) in the stale arena" % (i + 1, label))
        assert arena.taken > 0


@pytest.mark.gpu
def test_stale_arena_3d_persistent():
    big, small = (2, 20, 30, 200), (1, 8, 8, 64)
    assert _pers(*big, 12) and _pers(*big, 3) and _pers(*big, 12, 3) and _fused_bwd3d(*big, 12) and _pers(*small, 12)
    X = _in3d(*big, 101)
    Y = _in3d(*big, 102)
    M = _in3d(*big, 103, C=3)
    Fm = _in3d(*big, 104, raw=True, mask=True, signed=False)
    A = _in3d(*big, 105, raw=True)
    S = _in3d(*small, 106)
    fwd = lambda n: (lambda g, h, s, go: (F.cspn3d_forward(g, h, None, n, "none", "persistent"),))
    _run_sequence([
        ("forward n = 12 on X", fwd(12), X, big),
        ("forward n = 12 on Y: the same tags in flight", fwd(12), Y, big),
        ("forward n = 3 on X: the arena holds tags higher than any it will write", fwd(3), X, big),
        ("multi-channel C = 3", lambda g, h, s, go: (F.cspn3d_forward_multi(g, h, 12),), M, big),
        ("the folded mode with a mask", lambda g, h, s, go: (F.cspn3d_forward(g, h, s, 12, "8sum_abs", "persistent"),), Fm),
        ("absnorm", lambda g, h, s, go: (F.cspn3d_forward_absnorm(g, h, 12, "persistent"),), A, big),
        ("cspn3d_backward: the transposed instance", lambda g, h, s, go: F.cspn3d_backward(g, h, go, 12), X),
        ("forward n = 12 on a smaller volume: fewer workgroups indexed than were left dirty", fwd(12), S, small),
        ("the first shape again", fwd(12), X, big)], 4 * 2 * 3 * 20 * 30 * 200, three_d=True)


@pytest.mark.gpu
def test_stale_arena_2d():
    steps = []
    for W in (516, 260):   # the wider one first: the narrower finds its leftovers
        P = _in2d(2, 41, W - 2, "8sum", True, seed=W)
        R = _in2d(2, 41, W, "8sum", True, seed=W + 1, grad=True)
        assert _auto2d(2, 41, W - 2, 24) == _lib.ALGOS["fused_padded"] and cspn_amd.cspn2d_history_bytes(2, 41, W, 24) > 0
        steps += [("padded forward, W = %d" % (W - 2), lambda g, h, s: (F.cspn2d_forward(g, h, s, 24, "8sum"),), P),
                  ("ring backward, W = %d" % W, lambda g, h, s, go: F.cspn2d_backward(g, h, s, go, 24, "8sum"), R),
                  ("history backward, W = %d" % W, _history_call(12, "8sum"), R),
                  ("per-step backward, W = %d" % (W - 2), lambda g, h, s, go: F.cspn2d_backward(g, h, s, go, 5, "8sum"), _in2d(2, 41, W - 2, "8sum", True, seed=W + 2, grad=True)),
                  ("forward n = 36 (the ping plane), W = %d" % W, lambda g, h, s, go: (F.cspn2d_forward(g, h, s, 36, "8sum"),), R)]
    _run_sequence(steps, 4 * 2 * 41 * 516)


@pytest.mark.gpu
def test_stale_arena_kxk():
    steps = []
    for K in (5, 7):
        I = _kxk_inputs("none", K, 35, 196, F32, 200 + K)
        steps += [("forward K = %d" % K, lambda g, x, s, go, K=K: (F.cspn2d_forward_kxk(g, x, K, 4),), I),
                  ("backward K = %d" % K, lambda g, x, s, go, K=K: F.cspn2d_backward_kxk(g, x, go, K, 4), I)]
    J = _kxk_inputs("absnorm", 5, 67, 70, F16, 210)
    N = _kxk_inputs("norm", 7, 35, 196, F32, 211)
    steps += [("absnorm backward K = 5 (the 1 / S plane)", lambda g, x, s, go: F.cspn2d_backward_kxk_absnorm(g, x, go, 5, 3), J),
              ("norm forward K = 7", lambda g, x, s, go: (F.cspn2d_forward_kxk_norm(g, x, s, 7, 3, "8sum"),), N),
              ("norm backward K = 7", lambda g, x, s, go: F.cspn2d_backward_kxk_norm(g, x, s, go, 7, 3, "8sum"), N),
              ("forward K = 5 again", lambda g, x, s, go: (F.cspn2d_forward_kxk(g, x, 5, 4),), steps[0][2])]
    _run_sequence(steps, 4 * 2 * 2 * 35 * 196)


@pytest.mark.gpu
def test_stale_arena_heads():
    H, W = HEAD_SHAPE[4:]
    steps = []
    for P, dt, gd in ((8, F32, None), (48, F32, None), (24, BF16, None), (8, F16, F32)):
        I = _head_inputs(P, dt, 300 + P)
        steps += [("forward, %d planes %s" % (P, dt), lambda x, wg, wb, gg, gb, gd=gd: T.guidance_heads(x, wg, wb, H, W, guidance_dtype=gd), I),
                  ("backward, %d planes %s" % (P, dt), lambda x, wg, wb, gg, gb, gd=gd: T.guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=gd), I)]
    steps.append(("forward, 8 planes again", steps[0][1], steps[0][2]))
    _run_sequence(steps, 4 * 3 * 48 * H * W)
