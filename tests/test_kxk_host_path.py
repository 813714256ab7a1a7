"""The one host path of the folded (cspn2d_*_kxk_norm) and the assembling (cspn2d_*_kxk_assemble) K x K calls, pinned or not: the eight public
functions of cspn_amd.functional and the four autograd Functions of cspn_amd.cspn against the C ABI itself, called here through _lib.symbol with
the arguments as include/cspn_amd.h declares them and a workspace of the test's own -- bit for bit (torch.equal): the host path adds no arithmetic
and these backwards are deterministic."""
import ctypes
import inspect
import itertools

import pytest
import torch

import cspn_amd
import cspn_amd.cspn
from cspn_amd import _lib
from cspn_amd import functional as F

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CONTRACTS = ("norm", "assemble")
ENTRIES = ("f32", "g16", "dil", "pin")   # the suffix of the entry point a case must reach
PUBLIC = ["cspn2d_%s_kxk_%s%s" % (way, contract, pin) for contract in CONTRACTS for pin in ("", "_pin") for way in ("forward", "backward")]
CLASSES = ["_CSPN2dKxKNormFunction", "_CSPN2dKxKNormPinFunction", "_CSPN2dKxKAssembleFunction", "_CSPN2dKxKAssemblePinFunction"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_one_implementation_and_nothing_is_left_behind():
    for name in PUBLIC:
        source = inspect.getsource(getattr(F, name))
        assert "_launch(" not in source and "torch.empty" not in source and "_lib.symbol" not in source, name
        assert source.count("_fold_forward(" if "forward" in name else "_fold_backward(") == 1, name
    source = inspect.getsource(F)
    assert source.count("max(hb // 4, 1)") == 1
    assert source.count("history.numel() * history.element_size()") == 1
    for gone in ("_kxk_norm_args", "_assemble_args"):
        assert gone not in source, gone
    base = cspn_amd.cspn._CSPN2dKxKFoldFunction
    for name in CLASSES:
        cls = getattr(cspn_amd.cspn, name)
        assert issubclass(cls, base) and cls is not base and cls.backward is base.backward and "backward" not in vars(cls), name
        body = inspect.getsource(cls.forward)
        assert "_CSPN2dKxKFoldFunction.run(" in body and "F.cspn2d" not in body and "F._fold" not in body, name   # its own parameter list, the shared body
    functions = [c for c in vars(cspn_amd.cspn).values() if isinstance(c, type) and issubclass(c, base) and c is not base]
    assert sorted(c.__name__ for c in functions) == sorted(CLASSES)


def test_every_name_the_path_can_build_is_in_the_symbol_table():
    assert set(F._FOLD_NAMES) == {False, True}
    names = set()
    for row in F._FOLD_NAMES.values():
        names.update((row.history_bytes, row.forward_workspace_bytes, row.backward_workspace_bytes))
        for stem, dt, dilation in itertools.product((row.forward, row.backward), (None,) + tuple(_lib.DTYPES.values()), F.KXK_DILATIONS):
            names.update((F._kxk_entry(stem, dt, dilation)[0], F._pin_entry(stem, dt, dilation)[0]))
    want = {"cspn2d_%s_kxk_%s_%s" % (way, contract, entry) for way in ("forward", "backward") for contract in CONTRACTS for entry in ENTRIES}
    want |= {q % contract for contract in CONTRACTS for q in ("cspn2d_kxk_%s_history_bytes", "cspn2d_kxk_%s_workspace_bytes",
                                                               "cspn2d_backward_kxk_%s_workspace_bytes")}
    assert names == want and names <= set(_lib._SYMBOLS)


def _cpu_call(name, kernel_size=5, dilation=1, pin_shape=(1, 1, 6, 9), steps=(1, 3), grad_shape=(1, 2, 6, 9), grad_device="cpu"):
    """one of the eight functions on well-formed CPU tensors (K = 5, n_iter = 3), but for what the arguments spoil"""
    g, h, s = torch.rand(1, 24, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9)
    args = [g, h, s] + ([torch.rand(*pin_shape)] if name.endswith("_pin") else []) + ([torch.rand(1, 2, 6, 9), steps] if "assemble" in name else []) \
        + ([torch.rand(*grad_shape, device=grad_device)] if "backward" in name else [])
    return getattr(F, name)(*args, kernel_size=kernel_size, n_iter=3, dilation=dilation)


@pytest.mark.parametrize("name", PUBLIC)
def test_two_faults_at_once_raise_the_one_that_comes_first_in_the_one_order(name):
    """kernel_size, norm_type, n_iter and the shapes; the pin; conf and steps; the dilation; grad_out; the device"""
    with pytest.raises(ValueError, match="kernel_size"):
        _cpu_call(name, kernel_size=4, dilation=3)
    if name.endswith("_pin"):
        with pytest.raises(ValueError, match="pin_conf"):
            _cpu_call(name, pin_shape=(1, 1, 6, 8), dilation=3)
        if "assemble" in name:
            with pytest.raises(ValueError, match="pin_conf"):
                _cpu_call(name, pin_shape=(1, 1, 6, 8), steps=(3, 1))
    if "assemble" in name:
        with pytest.raises(ValueError, match="steps"):
            _cpu_call(name, steps=(3, 1), dilation=3)
    if "backward" in name:
        with pytest.raises(ValueError, match="dilation"):
            _cpu_call(name, dilation=3, grad_shape=(1, 1, 6, 9))
        with pytest.raises(ValueError, match="grad_out"):
            _cpu_call(name, grad_shape=(1, 1, 6, 9), grad_device="meta")
        with pytest.raises(ValueError, match="same device"):
            _cpu_call(name, grad_device="meta")
    with pytest.raises(ValueError, match="dilation"):
        _cpu_call(name, dilation=3)
    with pytest.raises(cspn_amd.CspnError):   # well-formed: the engine is reached, and it is GPU-only
        _cpu_call(name)


# ---------------------------------------------------------------------------------------------------------------- GPU
N_ITER = 3
SHAPES = [(2, 3, 17, 65),    # the guarded scalar path: odd W, a partial tile
          (1, 1, 16, 64)]    # one whole vectorised tile
A, L = (0, 2, 3), (3,)       # the steps of an assembling case
# (entry, contract, K, guidance dtype, dilation, sparse planes, norm, index into SHAPES, steps)
CASES = [
    ("f32", "norm", 5, F32, 1, None, "8sum", 0, None),
    ("f32", "norm", 3, F32, 1, "shared", "8sum_abs", 1, None),
    ("f32", "norm", 7, F32, 1, "per", "8sum", 0, None),
    ("g16", "norm", 5, F16, 1, "per", "8sum_abs", 0, None),
    ("g16", "norm", 7, BF16, 1, None, "8sum", 1, None),
    ("g16", "norm", 3, BF16, 1, "shared", "8sum", 0, None),
    ("dil", "norm", 3, F32, 2, "per", "8sum", 0, None),
    ("dil", "norm", 5, BF16, 2, None, "8sum_abs", 1, None),
    ("dil", "norm", 7, F16, 2, "shared", "8sum", 0, None),
    ("pin", "norm", 5, F32, 1, "shared", "8sum", 0, None),
    ("pin", "norm", 7, F16, 2, "per", "8sum_abs", 0, None),
    ("pin", "norm", 3, BF16, 1, "per", "8sum", 1, None),
    ("pin", "norm", 5, F32, 2, "shared", "8sum_abs", 1, None),
    ("f32", "assemble", 5, F32, 1, "shared", "8sum", 0, A),
    ("f32", "assemble", 7, F32, 1, None, "8sum_abs", 1, L),
    ("g16", "assemble", 3, F16, 1, "per", "8sum", 0, L),
    ("g16", "assemble", 5, BF16, 1, None, "8sum_abs", 1, A),
    ("dil", "assemble", 7, F32, 2, "per", "8sum", 0, A),
    ("dil", "assemble", 3, F16, 2, "shared", "8sum_abs", 1, A),
    ("dil", "assemble", 5, BF16, 2, None, "8sum", 0, L),
    ("pin", "assemble", 3, F32, 2, "shared", "8sum", 0, A),
    ("pin", "assemble", 5, F16, 1, "per", "8sum_abs", 0, L),
    ("pin", "assemble", 7, BF16, 2, "shared", "8sum", 1, A),
    ("pin", "assemble", 7, F32, 1, "per", "8sum_abs", 0, A),
]


def _case_id(c):
    entry, contract, K, dt, dil, sparse, norm, shape, steps = c
    return "-".join([contract, entry, "K%d" % K, str(dt).split(".")[1], "d%d" % dil, str(sparse), norm, "x".join(map(str, SHAPES[shape]))]
                    + (["s" + "".join(map(str, steps))] if steps else []))


def test_the_cases_cover_every_value_of_every_factor_and_reach_the_entry_point_they_name():
    assert 20 <= len(CASES) <= 28 and len(set(CASES)) == len(CASES)
    for contract in CONTRACTS:
        mine = [c for c in CASES if c[1] == contract]
        assert {c[0] for c in mine} == set(ENTRIES)
        for entry in ENTRIES:   # every entry point on both shapes, each contract
            assert {c[7] for c in mine if c[0] == entry} == {0, 1}, (contract, entry)
        for i, values in ((2, {3, 5, 7}), (3, {F32, F16, BF16}), (4, {1, 2}), (5, {None, "shared", "per"}), (6, {"8sum", "8sum_abs"})):
            assert {c[i] for c in mine} == values, (contract, i)
    assert {c[8] for c in CASES if c[1] == "assemble"} == {A, L} and all(c[8] is None for c in CASES if c[1] == "norm")
    assert all(s[-1] == N_ITER for s in (A, L))
    for entry, contract, K, dt, dil, sparse, norm, shape, steps in CASES:
        stem = "cspn2d_forward_kxk_" + contract
        if entry == "pin":
            assert sparse is not None                       # a pin needs a measurement
            reached = F._pin_entry(stem, _lib.DTYPES.get(str(dt).split(".")[1]), dil)[0]
        else:
            reached = F._kxk_entry(stem, _lib.DTYPES.get(str(dt).split(".")[1]), dil)[0]
        assert reached == stem + "_" + entry, (reached, entry)
    for entry in ("pin", "dil"):   # each on float32 and on 16-bit guidance; the pin at both dilations
        assert {c[3] == F32 for c in CASES if c[0] == entry} == {True, False}
    assert {c[4] for c in CASES if c[0] == "pin"} == {1, 2}


class _Case(object):
    """the tensors of a case on the GPU, made once and never written to"""

    def __init__(self, c):
        self.entry, self.contract, self.K, self.dtype, self.dilation, sparse, self.norm, shape, self.steps = c
        B, C, H, W = self.shape = SHAPES[shape]
        self.pinned, self.assembles = self.entry == "pin", self.contract == "assemble"
        gen = torch.Generator().manual_seed(1000 * self.K + 10 * W + CASES.index(c))
        self.g = torch.randn(B, self.K * self.K - 1, H, W, generator=gen).cuda().to(self.dtype)
        self.h = (torch.rand(B, C, H, W, generator=gen) * 10).cuda()
        self.sc = {None: 0, "shared": 1, "per": C}[sparse]
        self.s = self.p = self.cf = None
        if sparse:   # ~ 30 % measured, one value negative: the engine reads the sign (and, pinned, the value)
            s = (torch.rand(B, self.sc, H, W, generator=gen) < 0.3).float() * (torch.rand(B, self.sc, H, W, generator=gen) * 10 + 0.1)
            s.view(-1)[3] = -2.5
            self.s = s.cuda()
        if self.pinned:
            self.p = torch.rand(B, self.sc, H, W, generator=gen).cuda()
        if self.assembles:
            self.cf = torch.rand(B, len(self.steps), H, W, generator=gen).cuda()
        self.go = torch.randn(B, C, H, W, generator=gen).cuda()
        # what the public functions take behind sparse_depth, and the names of the gradients in the order every backward returns them
        self.extra = ((self.p,) if self.pinned else ()) + ((self.cf, self.steps) if self.assembles else ())
        self.grads = ["guidance", "blur"] + ["conf"] * self.assembles + ["sparse", "pin"] * self.pinned
        self.kw = dict(kernel_size=self.K, n_iter=N_ITER, norm_type=self.norm, dilation=self.dilation)
        suffix = "_pin" if self.pinned else ""
        self.forward = getattr(F, "cspn2d_forward_kxk_%s%s" % (self.contract, suffix))
        self.backward = getattr(F, "cspn2d_backward_kxk_%s%s" % (self.contract, suffix))
        self.function = getattr(cspn_amd.cspn, "_CSPN2dKxK%s%sFunction" % (self.contract.capitalize(), "Pin" if self.pinned else ""))

    # ---- the C ABI as include/cspn_amd.h declares it ----
    def _abi(self, way, middle, query, n_query):
        """guidance [, gate_dtype], blur, sparse [, pin_conf] [, conf, steps, T], `middle`, B, C, sparse_C, H, W, K [, dilation], n_iter, norm,
        workspace, its bytes, stream"""
        B, C, H, W = self.shape
        code = () if self.entry == "f32" else (_lib.DTYPES.get(str(self.dtype).split(".")[1], 0),)   # (0: float32, which _dil and _pin take too)
        steps = (ctypes.c_int * len(self.steps))(*self.steps) if self.assembles else None
        n = _lib.symbol(query)(B, C, self.sc, H, W, self.K, n_query)
        ws = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        rc = _lib.symbol("cspn2d_%s_kxk_%s_%s" % (way, self.contract, self.entry))(
            ptr(self.g), *code, ptr(self.h), ptr(self.s), *((ptr(self.p),) if self.pinned else ()),
            *((ptr(self.cf), steps, len(self.steps)) if self.assembles else ()),
            *(ptr(t) if isinstance(t, torch.Tensor) or t is None else t for t in middle),
            B, C, self.sc, H, W, self.K, *((self.dilation,) if self.entry in ("dil", "pin") else ()), N_ITER, _lib.NORM_TYPES[self.norm],
            ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, (way, rc, cspn_amd.load().cspn_last_error())

    def abi_forward(self, with_history):
        """-> out, history (None without one): float* out, float* history, size_t history_bytes"""
        B, C, H, W = self.shape
        out, hist, hb = torch.empty_like(self.h), None, 0
        if with_history:
            hb = _lib.symbol("cspn2d_kxk_%s_history_bytes" % self.contract)(B, C, H, W, self.K, N_ITER)
            hist = torch.zeros(max(hb // 4, 1), device="cuda")
        self._abi("forward", (out, hist, hb), "cspn2d_kxk_%s_workspace_bytes" % self.contract, 1 if with_history else N_ITER)
        return out, hist

    def abi_backward(self, hist):
        """-> the gradients in self.grads' order: history, history_bytes, grad_out, grad_guidance, grad_blur [, grad_conf] [, grad_sparse, grad_pin]"""
        like = dict(guidance=self.g, blur=self.h, conf=self.cf, sparse=self.s, pin=self.p)
        grads = [torch.empty_like(like[name]) for name in self.grads]
        self._abi("backward", (hist, hist.numel() * 4, self.go, *grads), "cspn2d_backward_kxk_%s_workspace_bytes" % self.contract, N_ITER)
        return grads


_CACHE = {}


def _case(c):
    """the case's tensors and what the ABI computes from them: computed once, shared by the tests, left unchanged"""
    if c not in _CACHE:
        t = _Case(c)
        t.out, t.hist = t.abi_forward(True)
        t.want = t.abi_backward(t.hist)
        _CACHE[c] = t
    return _CACHE[c]


def _same(got, want):
    assert len(got) == len(want)
    for a, r in zip(got, want):
        assert (a is None and r is None) or (a is not None and r is not None and a.dtype == r.dtype and torch.equal(a, r))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_each_public_call_is_the_raw_abi_call(c):
    t = _case(c)
    plain, _ = t.abi_forward(False)
    assert torch.equal(plain, t.out)
    _same([t.forward(t.g, t.h, t.s, *t.extra, **t.kw)], [t.out])
    _same(t.forward(t.g, t.h, t.s, *t.extra, return_history=True, **t.kw), (t.out, t.hist))
    assert t.want[0].dtype == t.dtype and all(g.dtype == F32 for g in t.want[1:])
    _same(t.backward(t.g, t.h, t.s, *t.extra, t.go, history=t.hist, **t.kw), t.want)
    _same(t.backward(t.g, t.h, t.s, *t.extra, t.go, history=None, **t.kw), t.want)     # runs its own forward for the history


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_gradient_subsets_with_and_without_a_history(c):
    t = _case(c)
    subsets = [("guidance",), ("blur",)] + [("conf",)] * t.assembles + [("sparse", "pin")] * t.pinned
    for subset in subsets:
        need = {"need_" + name: name in subset for name in t.grads}
        want = [g if name in subset else None for name, g in zip(t.grads, t.want)]
        _same(t.backward(t.g, t.h, t.s, *t.extra, t.go, history=t.hist, **need, **t.kw), want)
        _same(t.backward(t.g, t.h, t.s, *t.extra, t.go, history=None, **need, **t.kw), want)
    none = t.backward(t.g, t.h, t.s, *t.extra, t.go, **{"need_" + name: False for name in t.grads}, **t.kw)
    assert len(none) == len(t.grads) and all(g is None for g in none)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_each_autograd_function_is_the_raw_abi_call(c):
    t = _case(c)
    leaves = dict(guidance=t.g, blur=t.h, conf=t.cf, sparse=t.s, pin=t.p)
    leaves = {name: leaves[name].clone().requires_grad_(True) for name in t.grads}
    extra = ((leaves["pin"],) if t.pinned else ()) + ((leaves["conf"], t.steps) if t.assembles else ())
    y = t.function.apply(leaves["guidance"], leaves["blur"], leaves["sparse"] if t.pinned else t.s, *extra, t.K, N_ITER, t.norm, t.dilation)
    assert t.function.__name__ in type(y.grad_fn).__name__
    saved = y.grad_fn.saved_tensors
    assert saved[-1] is not None and torch.equal(saved[-1], t.hist)     # the history is kept, and it is the last of the saved tensors
    y.backward(t.go)
    _same([y.detach()] + [leaves[name].grad for name in t.grads], [t.out] + t.want)
    # only blur_depth asks for a gradient: no history is kept
    h = t.h.clone().requires_grad_(True)
    y = t.function.apply(t.g, h, t.s, *t.extra, t.K, N_ITER, t.norm, t.dilation)
    assert y.grad_fn.saved_tensors[-1] is None
    y.backward(t.go)
    _same([y.detach(), h.grad], [t.out, t.want[1]])
