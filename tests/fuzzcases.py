"""Seeded draws over the K x K engine's four contracts (cspn2d_kxk.hip), the 3D normalising / masked modes (cspn3d_*_norm*) and the four guidance-head
paths (cspn_head*.hip, past the 64-channel chunks of their backwards), each case checked against the float64 statement its family's own test file already trusts.  A plain helper module, like memguard.py and helpers.py; not collected.
tests/test_fuzz_statements.py commits one seed and runs it; `python tests/fuzzcases.py` is the longer soak (FUZZ_CASES, FUZZ_SEED as
tools/fuzz_parity.py reads them; or one descriptor as its argument, which replays that case).  DESIGN.md §4.3.

    draw(family, seed, count)    plain descriptors (named tuples of ints and strings) from random.Random(seed): no torch, no GPU
    inputs(case)                 CPU tensors from CPU generators seeded by the case, made by the family's own generators
    reference(case)              the family's float64 statement and its autograd gradients (imported, not restated)
    place(case, tensors)         each tensor on the device on its own: as allocated, or a contiguous view one element into a larger buffer
    run(case)                    the engine calls, through cspn_amd.functional
    check(case)                  run() and every assertion; no bound is defined here

Roles, one letter each: g the gate / guidance / guide, x the values (x, blur_depth, feat), s sparse_depth, c conf, o grad_out.  A descriptor's
`offset` names the roles placed one element off, its `need` (K x K) the gradients asked for: g, x, c.
The head family names its roles in full (HEAD_ROLES, joined with '+' in `offset`); its `need` is x, w or xw."""
import collections
import functools
import os
import random
import sys

FAMILIES = ("kxk", "3d", "head")
CONTRACTS = ("none", "norm", "absnorm", "assemble")
KERNELS = {"none": (5, 7), "norm": (3, 5, 7), "absnorm": (5, 7), "assemble": (3, 5, 7)}
ROLES = {"none": "gxo", "norm": "gxso", "absnorm": "gxo", "assemble": "gxsco", "3d": "gxso"}
NEEDS = {"none": ("g", "x", "gx"), "norm": ("g", "x", "gx"), "absnorm": ("g", "x", "gx"), "assemble": ("g", "x", "c", "gx", "gc", "xc", "gxc")}
DTYPES = ("float32", "float16", "bfloat16")
NORMS = ("8sum", "8sum_abs")
MASKS2D = ("none", "shared", "per")
MASKS3D = ("nomask", "mask", "mask_neg")
KXK_H = (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 35, 49)
KXK_W = (1, 2, 3, 5, 63, 64, 65, 66, 67, 68, 127, 128, 129, 130, 196, 259)
VOL_D = (1, 2, 3, 7, 8, 9, 17)
VOL_H = (1, 2, 7, 8, 9, 16, 17)
VOL_W = (1, 3, 4, 5, 8, 63, 64, 65, 68, 72, 130)
TILE_W, TILE_H = 64, 16          # the K x K kernels' tile
KXK_ELEMENTS, VOL_ELEMENTS = 40000, 30000
N_MAX, T_MAX = 6, 4

KxK = collections.namedtuple("KxK", "family index contract K dtype B C H W n norm mask steps need offset seed")
Vol = collections.namedtuple("Vol", "family index norm mask C dtype B D H W n algo offset seed")

# the guidance heads: path A cspn_guidance_head[_backward]_f32, B ..._kxk[_backward]_f32, C ..._kxk[_backward]_g16, D cspn_guidance_head[_backward]_g16
HEAD_PATHS = "ABCD"
HEAD_ROLES = ("x", "weight_guidance", "weight_blur", "grad_guidance", "grad_blur")
HEAD_PLANES = {"A": (8,), "B": (24, 48), "C": (24, 48), "D": (8,)}
HEAD_DTYPES = {"A": ("float32",), "B": ("float32",), "C": ("float16", "bfloat16"), "D": ("float16", "bfloat16")}
HEAD_NEEDS = ("x", "w", "xw")
HEAD_NORMS = ("none", "8sum", "8sum_abs")          # path A only: the normalisation fused behind the conv (grad off)
HEAD_C = (1, 7, 16, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 200)
HEAD_CLASSES = ("C <= 32", "C 33..64", "C 65..96", "C 97..128", "C > 128")   # chunks of 64 channels, one or two column blocks of 32 in the last
HEAD_W = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 100)
HEAD_H_MAX = 9
HEAD_ELEMENTS = 120000
HEAD_OFFSET_P = 0.25       # a free slot offsets each role with this probability: one case in four keeps every tensor as allocated
# dL/dW: (pixels of a tile, waves of a launch at most) as the host code has them -- cspn_head_backward.hip W2_TP, DW_MAX_WAVES; cspn_head_kxk.hip
# DW_TILE, 4 * DW_MAX_WG (cspn_head_kxk_common.h); cspn_head_g16_common.h DW_TILE for C and D.  tests/test_fuzz_statements.py reads them out of csrc
HEAD_DW = {"A": (32, 2048), "B": (8, 1024), "C": (16, 1024), "D": (16, 1024)}
HEAD_MANY = {"A": (3, 65, 33), "B": (2, 97, 33), "C": (2, 97, 33), "D": (2, 97, 33)}   # B, C, w of the slot with more tiles than waves; h is the smallest that has

Head = collections.namedtuple("Head", "family index path planes dtype B C h w oh ow blur norm need w16 offset seed")


# ---- the draw: pure Python ----
class _Deck(object):
    """every value of an axis equally often, in no fixed order against the other axes: the values are shuffled, dealt, and shuffled again"""

    def __init__(self, rnd, values):
        self.rnd, self.values, self.hand = rnd, list(values), []

    def deal(self):
        if not self.hand:
            self.hand = list(self.values)
            self.rnd.shuffle(self.hand)
        return self.hand.pop()


def _some(rnd, roles):
    return "".join(r for r in roles if rnd.random() < 0.5)


def _draw_kxk(rnd, count):
    """case j belongs to contract j % 4; within a contract K, the gate dtype and the need_* subset are dealt from decks, slot r < len(roles) offsets
    role r alone at a width the vector kernels take, the next two slots are tile grids of >= 3 x 2 and >= 2 x 3 (columns x rows), the rest is free"""
    decks = {c: {"K": _Deck(rnd, KERNELS[c]), "dtype": _Deck(rnd, DTYPES), "need": _Deck(rnd, NEEDS[c])} for c in CONTRACTS}
    w4 = [w for w in KXK_W if w % 4 == 0]
    cases = []
    for j in range(count):
        contract, slot = CONTRACTS[j % 4], j // 4
        roles = ROLES[contract]
        masked = contract in ("norm", "assemble")
        K, dtype, need = (decks[contract][a].deal() for a in ("K", "dtype", "need"))
        while True:
            B, C, H, W = rnd.randint(1, 3), rnd.randint(1, 4), rnd.choice(KXK_H), rnd.choice(KXK_W)
            if slot < len(roles):
                W = rnd.choice(w4)
            elif slot == len(roles):       # >= 3 tile columns, >= 2 tile rows
                W, H = rnd.choice([w for w in KXK_W if w > 2 * TILE_W]), rnd.choice([h for h in KXK_H if h > TILE_H])
            elif slot == len(roles) + 1:   # >= 3 tile rows, >= 2 tile columns
                W, H = rnd.choice([w for w in KXK_W if w > TILE_W]), rnd.choice([h for h in KXK_H if h > 2 * TILE_H])
            grid = slot in (len(roles), len(roles) + 1)
            if grid and B * C * H * W > KXK_ELEMENTS:
                continue                   # a grid slot keeps its H: other B, C
            while B * C * H * W > KXK_ELEMENTS:
                H //= 2
            if contract != "none" and H * W <= (2 if masked else 1):
                continue                   # one pixel has no neighbour in range: S = 0, NaN (pinned elsewhere); two pixels of the sited contract have
            break                          # one each, its gate is +-1 whatever the guidance, dL/dguidance = 0 and a relative bound has no scale
        n = rnd.randint(1, N_MAX)
        norm = rnd.choice(NORMS) if masked else ""
        mask = rnd.choice(MASKS2D) if masked else "none"
        steps = ""
        if contract == "assemble":
            T = rnd.randint(1, min(T_MAX, n + 1))
            steps = ",".join(str(s) for s in sorted(rnd.sample(range(n), T - 1)) + [n])
        if slot < len(roles):
            offset = roles[slot]
            if offset == "s" and mask == "none":
                mask = rnd.choice(MASKS2D[1:])
        else:
            offset = _some(rnd, roles)
        if mask == "none":
            offset = offset.replace("s", "")
        cases.append(KxK("kxk", j, contract, K, dtype, B, C, H, W, n, norm, mask, steps, need, offset, rnd.randrange(1 << 30)))
    return cases


def _draw_3d(rnd, count):
    """norm, mask and the guidance dtype are dealt from decks; case 0 offsets the guidance alone, case 1 feat alone (at widths the vector kernels
    take), cases 2 and 3 are volumes of partial tiles that the persistent kernel takes both ways, the rest is free"""
    decks = {"norm": _Deck(rnd, NORMS), "mask": _Deck(rnd, MASKS3D), "dtype": _Deck(rnd, DTYPES)}
    cases = []
    for j in range(count):
        norm, mask, dtype = (decks[a].deal() for a in ("norm", "mask", "dtype"))
        roles = ROLES["3d"] if mask != "nomask" else ROLES["3d"].replace("s", "")
        while True:
            B, C = rnd.randint(1, 2), rnd.randint(1, 4)
            D, H, W = rnd.choice(VOL_D), rnd.choice(VOL_H), rnd.choice(VOL_W)
            n = rnd.randint(1, N_MAX)
            offset = _some(rnd, roles)
            if j < 2:
                W, offset = rnd.choice([w for w in VOL_W if w % 4 == 0]), "gx"[j]
            elif j < 4:
                W, n, offset = rnd.choice([w for w in VOL_W if w % 4 == 0 and w >= 64]), rnd.randint(3, N_MAX), ""
                D, H = rnd.choice([d for d in VOL_D if d % 8]), rnd.choice([h for h in VOL_H if h % 8])
                if B * C * D * H * W > VOL_ELEMENTS:
                    continue
            while B * C * D * H * W > VOL_ELEMENTS:
                if D >= H:
                    D //= 2
                else:
                    H //= 2
            if D * H * W <= 2:
                continue                   # one voxel: S = 0; two: one neighbour each, dL/dguidance = 0 (as in 2D)
            break
        cases.append(Vol("3d", j, norm, mask, C, dtype, B, D, H, W, n, rnd.choice(("auto", "stepwise")), offset, rnd.randrange(1 << 30)))
    return cases


def chunk_class(C):
    """which of HEAD_CLASSES: how many 64-channel chunks the backwards' host loops run, and whether the last has one column block or two"""
    return 0 if C <= 32 else 1 if C <= 64 else 2 if C <= 96 else 3 if C <= 128 else 4


def head_out_size(case):
    return (case.oh, case.ow) if case.oh else (2 * case.h, 2 * case.w)


def head_tiles(case):
    """the tiles of the path's dL/dW launch, as its host code counts them"""
    H, W = head_out_size(case)
    px = HEAD_DW[case.path][0]
    return case.B * min((H + 1) // 2, case.h) * ((min((W + 1) // 2, case.w) + px - 1) // px)


def offsets_of(case):
    return tuple(case.offset.split("+")) if case.offset else ()


def _draw_head(rnd, count):
    """case j belongs to path 'ABCD'[j % 4]; within a path the plane count, dtype, need_*, norm (A), 16-bit weights (C, D) and C are dealt from decks
    (C over every class of HEAD_CLASSES), slot r < 5 offsets role r alone at W % 4 = 0 and an exact 2x output (the fast stores stay on), slot 5 has
    more dL/dW tiles than the launch has waves at C > 64 and asks for both gradients, slots 3, 7, 11 ... have no blur head, the rest is free"""
    decks = {p: {"planes": _Deck(rnd, HEAD_PLANES[p]), "dtype": _Deck(rnd, HEAD_DTYPES[p]), "need": _Deck(rnd, HEAD_NEEDS), "norm": _Deck(rnd, HEAD_NORMS),
                 "w16": _Deck(rnd, (0, 1)), "C": _Deck(rnd, HEAD_C)} for p in HEAD_PATHS}
    even = [w for w in HEAD_W if w % 2 == 0]
    cases = []
    for j in range(count):
        path, slot = HEAD_PATHS[j % 4], j // 4
        planes, dtype = (decks[path][a].deal() for a in ("planes", "dtype"))
        need = decks[path]["need"].deal() if slot != 5 else "xw"      # (the slot of many tiles asks for both gradients)
        norm = decks[path]["norm"].deal() if path == "A" else ""
        w16 = decks[path]["w16"].deal() if path in "CD" else 0
        blur = int(slot % 4 != 3)
        B, h, w = rnd.randint(1, 3), rnd.randint(1, HEAD_H_MAX), rnd.choice(HEAD_W)
        exact = rnd.random() < 0.4
        if slot == 5:                       # more tiles than waves, two chunks: the smallest h that has
            B, C, w = HEAD_MANY[path]
            px, waves = HEAD_DW[path]
            exact, h = True, waves // (B * ((w + px - 1) // px)) + 1
        else:
            C = decks[path]["C"].deal()
            if slot < len(HEAD_ROLES):
                w, exact = rnd.choice(even), True
            while B * C * h * w > HEAD_ELEMENTS:
                h //= 2
        oh, ow = (0, 0) if exact else (rnd.randint(max(1, 2 * h - 3), 2 * h), rnd.randint(max(1, 2 * w - 3), 2 * w))
        roles = [r for r in HEAD_ROLES if blur or not r.endswith("blur")]
        if slot < len(HEAD_ROLES):
            offset = HEAD_ROLES[slot]
            assert offset in roles
            if offset.startswith("weight"):
                w16 = 0                     # (16-bit weights reach the engine as fresh .float() copies: their own placement would not)
        elif slot == 5:
            offset = ""
        else:
            offset = "+".join(r for r in roles if rnd.random() < HEAD_OFFSET_P)
        cases.append(Head("head", j, path, planes, dtype, B, C, h, w, oh, ow, blur, norm, need, w16, offset, rnd.randrange(1 << 30)))
    return cases


def draw(family, seed, count):
    """`count` descriptors of `family` ('kxk', '3d' or 'head'): the same arguments always give the same list"""
    if family not in FAMILIES:
        raise ValueError("family must be one of %s, got %r" % (FAMILIES, family))
    rnd = random.Random("%s/%d" % (family, seed))
    return {"kxk": _draw_kxk, "3d": _draw_3d, "head": _draw_head}[family](rnd, count)


def steps_of(case):
    return tuple(int(s) for s in case.steps.split(",")) if case.steps else ()


def takes_persistent(case):
    """a 3D case that algo 'persistent' must take: whole quads, at least one tile wide, every tensor as allocated, n >= 2 (the backward: n >= 3)"""
    return case.family == "3d" and case.W % 4 == 0 and case.W >= 64 and case.n >= 2 and not case.offset


# ---- inputs and the float64 statements: torch on the CPU ----
def _torch_dtype(name):
    import torch
    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[name]


def inputs(case):
    """{role: CPU tensor or None}; g in the case's dtype, everything else float32"""
    import torch
    dt = _torch_dtype(case.dtype)
    if case.family == "head":
        return _head_inputs(case)
    if case.family == "3d":
        from test_3d_norm_multi import _inputs
        g, x, s, o = _inputs((case.B, case.D, case.H, case.W), case.C, case.seed, mask=case.mask)
        return {"g": g.to(dt), "x": x, "s": s, "o": o}
    B, C, H, W, K = case.B, case.C, case.H, case.W, case.K
    t = {"s": None, "c": None}
    if case.contract == "none":
        from test_kernel_size import _gates, _values
        t.update(g=_gates(B, K, H, W, case.seed), x=_values(B, C, H, W, case.seed + 1), o=_values(B, C, H, W, case.seed + 2))
    elif case.contract == "absnorm":
        from test_kxk_absnorm import _guide, _values
        t.update(g=_guide(B, K, H, W, case.seed), x=_values(B, C, H, W, case.seed + 1), o=_values(B, C, H, W, case.seed + 2))
    else:
        from test_kxk_norm import _inputs
        t["g"], t["x"], t["s"] = _inputs(B, C, H, W, K, None if case.mask == "none" else case.mask, case.seed)
        t["o"] = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(case.seed + 2))
        if case.contract == "assemble":
            from test_kxk_assemble import _conf
            t["c"] = _conf(B, len(steps_of(case)), H, W, case.seed + 1)
    t["g"] = t["g"].to(dt)
    return t


def _head_inputs(case):
    """as the head files make them: x randn, the weights randn / (3 sqrt C), the gradients randn, each from its own generator seeded by the case.  x in the
    case's dtype; the weights float32 masters, or (w16) tensors of x's dtype; grad_guidance in x's dtype on path C (what cspn2d_backward_kxk_norm hands
    back), float32 elsewhere; grad_blur float32; without a blur head weight_blur and grad_blur are None"""
    import torch
    dt = _torch_dtype(case.dtype)
    B, C, h, w, P = case.B, case.C, case.h, case.w, case.planes
    H, W = head_out_size(case)
    shapes = ((B, C, h, w), (P, C, 3, 3), (1, C, 3, 3), (B, P, H, W), (B, 1, H, W))
    t = {r: torch.randn(*s, generator=torch.Generator().manual_seed(case.seed + i)) for i, (r, s) in enumerate(zip(HEAD_ROLES, shapes))}
    for r in ("weight_guidance", "weight_blur"):
        t[r] = t[r] / (3.0 * C ** 0.5)
        if case.w16:
            t[r] = t[r].to(dt)
    t["x"] = t["x"].to(dt)
    if case.path == "C":
        t["grad_guidance"] = t["grad_guidance"].to(dt)
    if not case.blur:
        t["weight_blur"] = t["grad_blur"] = None
    return t


HEAD_OUTPUTS = ("guidance", "blur")
HEAD_GRADS = ("x", "weight_guidance", "weight_blur")


def _head_statement(case, dtype):
    """tests/test_head_kxk.py's statement on the operands rounded the way the path's own file rounds them (test_head_kxk_g16._reference on C,
    test_head_g16._case on D: whatever the engine takes or rounds to x's dtype dt is rounded to dt first; nothing on A and B) ->
    ({guidance, blur}, {x, weight_guidance, weight_blur}), None without a blur head.  float64: statement_grads itself"""
    import torch
    from test_head_kxk import statement as head_statement, statement_grads
    dt = _torch_dtype(case.dtype)
    t = inputs(case)
    x, wg, wb, gg, gb = (t[r].to(dt).double() if t[r] is not None else None for r in HEAD_ROLES)   # (every one of these widenings is exact)
    if dtype == torch.float64:
        g, b, dx, dwg, dwb = statement_grads(x, wg, wb, gg, gb, case.oh, case.ow)
    else:
        xs, wgs, wbs = (v.to(dtype).requires_grad_(True) if v is not None else None for v in (x, wg, wb))
        g, b = head_statement(xs, wgs, wbs, case.oh, case.ow)
        loss = (g * gg.to(dtype)).sum()
        if wb is not None:
            loss = loss + (b * gb.to(dtype)).sum()
        loss.backward()
        g, b, dx, dwg, dwb = g.detach(), (b.detach() if b is not None else None), xs.grad, wgs.grad, (wbs.grad if wbs is not None else None)
    return dict(zip(HEAD_OUTPUTS, (g, b))), dict(zip(HEAD_GRADS, (dx, dwg, dwb)))


# the heads' bounds, by reference: max |a - ref| / max |ref| of tests/test_head_kxk.py::_check_all (A: tests/test_head.py, the same figures) for the
# float32 results, test_head_kxk_g16._err16 <= 1 with the file's p for a result stored in 16 bits (guidance on C, dL/dx on C and D; test_head_g16._check)
HEAD_REL = {"guidance": 1e-5, "blur": 1e-5, "x": 1e-5, "weight_guidance": 2e-5, "weight_blur": 2e-5}
HEAD_NORMALISED = 2e-5     # tests/test_head.py::test_head_fuzzed_shapes_vs_oracle: |gate_wb - cspn2d_normalize(statement)| where both are finite


def head_sixteen(case):
    """the results the path stores in x's 16-bit dtype"""
    return {"A": (), "B": (), "C": ("guidance", "x"), "D": ("x",)}[case.path]


def head_fraction(case, name, a, ref):
    """how much of its bound result `name` uses against the float64 statement"""
    from test_head_kxk import _rel
    from test_head_kxk_g16 import DTS, _err16
    if name in head_sixteen(case):
        return _err16(a.cpu(), ref, DTS[case.dtype][1])
    return _rel(a, ref) / HEAD_REL[name]


def _normalised_fraction(got, want):
    """tests/test_head.py:161-166 on numpy arrays: the NaN pattern is equal, the rest within HEAD_NORMALISED"""
    import numpy as np
    assert np.array_equal(np.isnan(got), np.isnan(want)), "the NaN pattern of the normalised guidance differs"
    return float(np.nan_to_num(np.abs(got - want)).max()) / HEAD_NORMALISED


def _head_statement_fractions(case):
    """the float32 statement against the float64 one.  A result the engine stores in 16 bits is held to 2^-p |ref| + 1e-5 max |ref|; its one rounding
    may use the whole first term, so the UNROUNDED float32 statement is held to the second term alone: the same expression as for a float32 result"""
    import torch
    from test_head_kxk import _rel
    (ref_out, ref_grads), (out, grads) = reference(case), _head_statement(case, torch.float32)
    fwd = max(_rel(out[k], ref_out[k]) / HEAD_REL[k] for k in HEAD_OUTPUTS if ref_out[k] is not None)
    if case.norm not in ("", "none"):   # what a float32 guidance costs behind the normalisation (the C oracle's gate_wb, float32 itself)
        from oracle import cspn2d_gate_wb_oracle
        fwd = max(fwd, _normalised_fraction(cspn2d_gate_wb_oracle(out["guidance"].numpy(), case.norm),
                                            cspn2d_gate_wb_oracle(ref_out["guidance"].float().numpy(), case.norm)))
    return fwd, max(_rel(grads[k], ref_grads[k]) / HEAD_REL[k] for k in HEAD_GRADS if ref_grads[k] is not None)


def finite(ref):
    """every tensor of a reference() is finite"""
    every = []
    for part in ref:
        every += list(part.values()) if isinstance(part, dict) else [part]
    return all(bool(v.isfinite().all()) for v in every if v is not None)


def statement(case, dtype):
    """the family's statement in `dtype` on the case's inputs (a 16-bit g widened exactly) -> (out, {role: gradient})"""
    if case.family == "head":
        return _head_statement(case, dtype)
    t = inputs(case)
    leaf = lambda v: v.float().to(dtype).requires_grad_(True)   # noqa: E731
    g, x = leaf(t["g"]), leaf(t["x"])
    s = t["s"].to(dtype) if t["s"] is not None else None
    leaves = {"g": g, "x": x}
    if case.family == "3d":
        from test_3d_norm_multi import _statement
        out = _statement(g, x, s, case.n, case.norm)
    elif case.contract == "none":
        from test_kernel_size import _torch_noneKxK
        out = _torch_noneKxK(g, x, case.K, case.n)
    elif case.contract == "absnorm":
        from test_kxk_absnorm import _statement
        out = _statement(g, x, case.K, case.n)
    elif case.contract == "norm":
        from test_kxk_norm import torch_kxk_norm
        out = torch_kxk_norm(g, x, s, case.K, case.n, case.norm)
    else:
        from test_kxk_assemble import torch_kxk_assemble
        leaves["c"] = leaf(t["c"])
        out = torch_kxk_assemble(g, x, s, leaves["c"], steps_of(case), case.K, case.norm)
    out.backward(t["o"].to(dtype))
    return out.detach(), {r: v.grad for r, v in leaves.items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """the float64 output and its autograd gradients: computed once per case, never written"""
    import torch
    return statement(case, torch.float64)


# ---- the project's bounds, by reference ----
def bounds(case):
    """(forward, gradient) as (rtol, atol_frac) of helpers.assert_close: its defaults forward; tests/test_backward.py's _check for the K x K
    gradients, tests/test_backward3d_norm.py's for the 3D ones"""
    import helpers
    if case.family == "3d":
        from test_backward3d_norm import GFLOOR, GTOL
    else:
        from test_backward import GFLOOR, GTOL
    return (helpers.RTOL, helpers.ATOL_FRAC), (GTOL, GFLOOR)


def fraction(a, b, bound, what=""):
    """how much of `bound` a uses against b: helpers.assert_close's two conditions, the larger of the two ratios (it asserts both <= 1)"""
    import helpers
    err, worst = helpers.assert_close(a, b, what, rtol=bound[0], atol_frac=bound[1])
    return max(worst, err / bound[0])


def statement_fractions(case):
    """the float32 statement on the CPU against the float64 one, as fractions of the case's bounds -> (forward, gradients): what a correct
    float32 evaluation costs, so that the rest of a bound is the kernel's"""
    import torch
    if case.family == "head":
        return _head_statement_fractions(case)
    ref, ref_grads = reference(case)
    out, grads = statement(case, torch.float32)
    fwd, grad = bounds(case)
    return (fraction(out.numpy(), ref.numpy(), fwd, "%r float32 statement out" % (case,)),
            max(fraction(grads[r].numpy(), ref_grads[r].numpy(), grad, "%r float32 statement d/d%s" % (case, r)) for r in sorted(grads)))


# ---- placement and the engine calls: the GPU ----
def _one_off(t):
    """a contiguous device view of t's contents one element into a larger buffer (test_kxk_norm._misaligned; for 16 bits test_kxk_assemble's)"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % (16 if t.element_size() == 4 else 8) == t.element_size()
    return v


def place(case, tensors):
    """{role: device tensor or None}: each tensor on its own, one element off where the case's `offset` names its role, else as allocated"""
    off = offsets_of(case) if case.family == "head" else case.offset
    return {r: None if t is None else (_one_off(t) if r in off else t.cuda()) for r, t in tensors.items()}


def _widened(case, g16):
    """g16.float(), placed as the case places g: one element off a 16-byte boundary takes the same guarded scalar kernels (and, in 3D, keeps
    'auto' off the persistent sweeps) as one element off an 8-byte boundary does in 16 bits.  The project claims the float32 call's bits on the
    same path, not the aligned placement's bits for a misaligned one"""
    return _one_off(g16.float()) if "g" in case.offset else g16.float()


def bits(a, b):
    """the same dtype, shape and bit pattern"""
    import torch
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _calls(case):
    """(forward(t, return_history), backward(t, history, need)) of the K x K case's contract; need: one bool per gradient"""
    from cspn_amd import functional as F
    K, n, norm, steps = case.K, case.n, case.norm, steps_of(case)
    if case.contract in ("none", "absnorm"):
        f, b = (F.cspn2d_forward_kxk, F.cspn2d_backward_kxk) if case.contract == "none" else (F.cspn2d_forward_kxk_absnorm, F.cspn2d_backward_kxk_absnorm)
        return (lambda t, h=False: f(t["g"], t["x"], K, n, return_history=h)), (lambda t, hist, need: b(t["g"], t["x"], t["o"], K, n, hist, *need))
    if case.contract == "norm":
        return ((lambda t, h=False: F.cspn2d_forward_kxk_norm(t["g"], t["x"], t["s"], K, n, norm, return_history=h)),
                (lambda t, hist, need: F.cspn2d_backward_kxk_norm(t["g"], t["x"], t["s"], t["o"], K, n, norm, hist, *need)))
    return ((lambda t, h=False: F.cspn2d_forward_kxk_assemble(t["g"], t["x"], t["s"], t["c"], steps, K, n, norm, return_history=h)),
            (lambda t, hist, need: F.cspn2d_backward_kxk_assemble(t["g"], t["x"], t["s"], t["c"], steps, t["o"], K, n, norm, hist, *need)))


def _grad_roles(case):
    return "gxc" if case.family == "kxk" and case.contract == "assemble" else "gx"


def _run_kxk(case):
    import torch
    from cspn_amd import functional as F
    fwd, bwd = _calls(case)
    roles = _grad_roles(case)
    every = (True,) * len(roles)
    t = place(case, inputs(case))
    before = {r: v.clone() for r, v in t.items() if v is not None}
    res = {"placed": t, "before": before}
    res["out"] = fwd(t)
    res["out_again"] = fwd(t)
    res["out_hist"], hist = fwd(t, True)
    kept = hist.clone() if hist is not None else None
    res["grads"] = bwd(t, hist, every)
    res["grads_again"] = bwd(t, hist, every)
    res["grads_no_history"] = bwd(t, None, every)
    res["grads_subset"] = bwd(t, hist, tuple(r in case.need for r in roles))
    res["history"], res["history_before"] = hist, kept
    if case.dtype != "float32":
        t32 = dict(t, g=_widened(case, t["g"]))
        res["out32"] = fwd(t32)
        res["out32_hist"], res["history32"] = fwd(t32, True)
        res["grads32"] = bwd(t32, res["history32"], every)
    if case.contract == "assemble" and len(steps_of(case)) == 1:   # one collected level, conf = 1: the depth-completion engine
        one = dict(t, c=torch.ones_like(t["x"][:, :1]))
        res["unit_out"], res["unit_history"] = fwd(one, True)
        res["unit_grads"] = bwd(one, res["unit_history"], every)
        res["norm_out"], res["norm_history"] = F.cspn2d_forward_kxk_norm(t["g"], t["x"], t["s"], case.K, case.n, case.norm, return_history=True)
        res["norm_grads"] = F.cspn2d_backward_kxk_norm(t["g"], t["x"], t["s"], t["o"], case.K, case.n, case.norm, res["norm_history"])
    torch.cuda.synchronize()
    return res


def _multi_entry_points(case, t):
    """a C = 1 call through cspn3d_forward_norm_multi_* / cspn3d_backward_norm_multi_*, which the Python front-end never makes"""
    import torch
    from cspn_amd import _lib
    from cspn_amd import functional as F
    g, x, s, o = t["g"], t["x"], t["s"], t["o"]
    dt = () if case.dtype == "float32" else (_lib.DTYPES[case.dtype],)
    kind = "f32" if case.dtype == "float32" else "g16"
    dims = (case.B, 1, case.D, case.H, case.W, case.n, _lib.NORM_TYPES[case.norm])
    algo = _lib.ALGOS_3D[case.algo]
    out, gg, gf = torch.empty_like(x), torch.empty_like(g), torch.empty_like(x)
    # (a misaligned guidance or feat takes the folding path, sized by cspn3d_workspace_bytes: what cspn3d_forward asks for then)
    query = ("cspn3d_workspace_bytes", case.B, case.D, case.H, case.W, case.n) if set("gx") & set(case.offset) else \
        ("cspn3d_forward_norm_multi_workspace_bytes", *dims, int(s is not None))
    F._launch("cspn3d_forward_norm_multi_" + kind, g.device, (F._ptr(g), *dt, F._ptr(x), F._ptr(s), F._ptr(out), *dims, algo), query)
    F._launch("cspn3d_backward_norm_multi_" + kind, g.device, (F._ptr(g), *dt, F._ptr(x), F._ptr(s), F._ptr(o), F._ptr(gg), F._ptr(gf), *dims, algo),
              ("cspn3d_backward_norm_multi_workspace_bytes", *dims, int(s is not None)))
    return out, (gg, gf)


def _run_3d(case):
    import torch
    from cspn_amd import functional as F
    n, norm = case.n, case.norm
    fwd = lambda t, algo=case.algo: F.cspn3d_forward_norm(t["g"], t["x"], t["s"], n, norm, algo)   # noqa: E731
    bwd = lambda t, algo=case.algo, **kw: F.cspn3d_backward_norm(t["g"], t["x"], t["s"], t["o"], n, norm, algo, **kw)   # noqa: E731
    t = place(case, inputs(case))
    res = {"placed": t, "before": {r: v.clone() for r, v in t.items() if v is not None}}
    res["out"], res["out_again"] = fwd(t), fwd(t)
    res["grads"], res["grads_again"] = bwd(t), bwd(t)
    res["grads_g_alone"] = bwd(t, need_feat=False)
    res["grads_x_alone"] = bwd(t, need_guidance=False)
    t32 = t
    if case.dtype != "float32":
        t32 = dict(t, g=_widened(case, t["g"]))
        res["out32"], res["grads32"] = fwd(t32), bwd(t32)
    if case.C == 1:
        res["multi_out"], res["multi_grads"] = _multi_entry_points(case, t)
    if takes_persistent(case):   # CspnError here if the persistent kernel declines
        res["auto_out"], res["persistent_out"] = fwd(t, "auto"), fwd(t, "persistent")
        res["persistent_out32"] = fwd(t32, "persistent")
        if n >= 3:
            res["auto_grads"], res["persistent_grads"] = bwd(t, "auto"), bwd(t, "persistent")
            res["persistent_grads32"] = bwd(t32, "persistent")
    F.cspn3d_check_status()
    return res


def _run_head(case):
    """through cspn_amd.train_utils.guidance_heads / guidance_heads_backward only"""
    import torch
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    kw = {"guidance_dtype": torch.float32} if case.path == "D" else {}
    oh, ow, off = case.oh, case.ow, offsets_of(case)
    t = place(case, inputs(case))
    res = {"placed": t, "before": {r: v.clone() for r, v in t.items() if v is not None}}
    fwd = lambda **o: guidance_heads(*(o.get(r, t[r]) for r in HEAD_ROLES[:3]), oh, ow, **kw)   # noqa: E731
    bwd = lambda need_x=True, need_w=True, **o: guidance_heads_backward(*(o.get(r, t[r]) for r in HEAD_ROLES), need_x=need_x, need_w=need_w, **kw)   # noqa: E731
    res["out"], res["out_again"] = fwd(), fwd()
    res["grads"], res["grads_again"] = bwd(), bwd()
    res["grads_subset"] = bwd("x" in case.need, "w" in case.need)
    if case.w16:    # the float32 masters of the 16-bit weights
        masters = {r: t[r].float() for r in HEAD_ROLES[1:3] if t[r] is not None}
        res["out_masters"], res["grads_masters"] = fwd(**masters), bwd(**masters)
    # one autograd step on leaves that share the placed tensors' memory; what reaches the backward as dL/dguidance and dL/dblur is autograd's own
    # (as allocated) copy of grad_guidance and grad_blur, so the manual call it is compared with takes copies of those two where the case offsets them
    leaves = [t[r].detach().requires_grad_(True) if t[r] is not None else None for r in HEAD_ROLES[:3]]
    g, b = guidance_heads(*leaves, oh, ow, **kw)
    loss = (g * t["grad_guidance"]).sum()
    if b is not None:
        loss = loss + (b * t["grad_blur"]).sum()
    loss.backward()
    res["autograd_out"] = (g.detach(), b.detach() if b is not None else None)
    res["autograd_grads"] = tuple(v.grad if v is not None else None for v in leaves)
    copies = {r: t[r].clone() for r in HEAD_ROLES[3:] if r in off}
    res["grads_for_autograd"] = bwd(**copies) if copies else res["grads"]
    # a misaligned x (C, D) or grad_guidance (C) gives the aligned tensor's bits: tests/test_head_g16.py, tests/test_head_kxk_g16.py
    twin = {r: t[r].clone() for r in (("x", "grad_guidance") if case.path == "C" else ("x",) if case.path == "D" else ()) if r in off}
    if twin:
        res["out_aligned"], res["grads_aligned"] = fwd(**twin), bwd(**twin)
    if case.norm not in ("", "none"):
        from cspn_amd import cspn2d_normalize
        with torch.no_grad():
            res["normalised"] = fwd_n = guidance_heads(t["x"], t["weight_guidance"], t["weight_blur"], oh, ow, norm_type=case.norm)
        assert fwd_n[0].dtype == torch.float32
        res["normalised_statement"] = cspn2d_normalize(reference(case)[0]["guidance"].float().cuda(), case.norm)
    torch.cuda.synchronize()
    return res


def _check_head(case):
    """The 16-bit kernels are not the float32 kernels on widened operands (they round the weights and the gradients to x's dtype and run other
    matrix-core instructions), so the K x K and 3D families' anchor 'bitwise the float32 call on the widened tensor' does not exist here: a 16-bit
    case is held to the statement on the rounded operands, under its own file's bounds"""
    import torch
    res = run(case)
    what = repr(case)
    dt = _torch_dtype(case.dtype)
    out, grads = res["out"], res["grads"]
    _same(res["out_again"], out, what + " forward, called twice")
    _same(res["grads_again"], grads, what + " backward, called twice")
    for i, r in enumerate(HEAD_GRADS):
        asked = ("x" if r == "x" else "w") in case.need
        assert bits(res["grads_subset"][i], grads[i] if asked else None), "%s need=%s: d/d%s is not %s" % (what, case.need, r, "the full call's" if asked else "None")
    assert out[0].dtype == (dt if case.path == "C" else torch.float32) and grads[0].dtype == dt, what + ": dtypes of guidance and dL/dx"
    if case.blur:
        assert out[1].dtype == torch.float32 and grads[2] is not None
    else:
        assert out[1] is None and grads[2] is None, what + ": a blur or a dL/dW_blur without a blur head"
    # 16-bit weights: the bits of their float32 masters' call, the weight gradients that call's .to(dt)
    out32, grads32 = out, grads
    if case.w16:
        out32, grads32 = res["out_masters"], res["grads_masters"]
        _same(out, out32, what + " 16-bit weights against their .float() masters, forward")
        assert bits(grads[0], grads32[0]), what + ": dL/dx with 16-bit weights against their .float() masters"
        for i in (1, 2):
            assert bits(grads[i], grads32[i].to(dt) if grads32[i] is not None else None), what + ": a 16-bit weight's gradient is not the float32 one .to(dtype)"
    assert all(v is None or v.dtype == torch.float32 for v in grads32[1:]), what
    _same(res["autograd_out"], out, what + " forward under autograd")
    _same(res["autograd_grads"], res["grads_for_autograd"], what + " .grad after one autograd step against guidance_heads_backward")
    if "out_aligned" in res:
        _same(res["out_aligned"], out, what + " forward: one element off against as allocated")
        _same(res["grads_aligned"], grads, what + " backward: one element off against as allocated")
    # against the float64 statement (without a blur head: the statement without one)
    ref_out, ref_grads = reference(case)
    assert finite((ref_out, ref_grads)), what + ": the float64 statement is not finite"
    used = {}
    for name, a, r in tuple(zip(HEAD_OUTPUTS, out32, (ref_out[k] for k in HEAD_OUTPUTS))) + tuple(zip(HEAD_GRADS, grads32, (ref_grads[k] for k in HEAD_GRADS))):
        assert (a is None) == (r is None), "%s: %s is None on one side only" % (what, name)
        if a is not None:
            key = name if name in HEAD_OUTPUTS else "d/d" + name
            used[key] = head_fraction(case, name, a, r)
            assert used[key] <= 1.0, "%s: %s uses %.3g of its bound" % (what, key, used[key])
    if "normalised" in res:
        assert bits(res["normalised"][1], out[1]), what + ": blur of the normalising call is not the raw call's"
        used["normalised"] = _normalised_fraction(res["normalised"][0].cpu().numpy(), res["normalised_statement"].cpu().numpy())
        assert used["normalised"] <= 1.0, "%s: the normalised guidance uses %.3g of its bound" % (what, used["normalised"])
    for r, v in res["before"].items():
        assert bits(res["placed"][r], v), "%s: the calls wrote input %r" % (what, r)
    return used


def run(case):
    """every engine call of the case -> {name: result}"""
    return {"kxk": _run_kxk, "3d": _run_3d, "head": _run_head}[case.family](case)


def _same(a, b, what):
    for i, (p, q) in enumerate(zip(a, b) if isinstance(a, tuple) else ((a, b),)):
        assert bits(p, q), "%s: other bits (result %d)" % (what, i)


def check(case):
    """run(case), then: the float32 results within the project's bounds of the float64 statement, the bitwise anchors the project claims, the
    inputs untouched -> {what: fraction of its bound}.  The head family: _check_head"""
    if case.family == "head":
        return _check_head(case)
    res = run(case)
    what = repr(case)
    roles = _grad_roles(case)
    ref, ref_grads = reference(case)
    fwd_bound, grad_bound = bounds(case)
    sixteen = case.dtype != "float32"
    used = {}
    # a second identical call; a subset of the gradients; a history that was handed in
    _same(res["out_again"], res["out"], what + " forward, called twice")
    _same(res["grads_again"], res["grads"], what + " backward, called twice")
    if case.family == "kxk":
        _same(res["out_hist"], res["out"], what + " forward that keeps its levels")
        _same(res["grads_no_history"], res["grads"], what + " backward without a history")
        for i, r in enumerate(roles):
            want = res["grads"][i] if r in case.need else None
            assert bits(res["grads_subset"][i], want), "%s need=%s: d/d%s is not %s" % (what, case.need, r, "the full call's" if r in case.need else "None")
        assert bits(res["history"], res["history_before"]), what + ": the backward wrote the history"
    else:
        assert res["grads_g_alone"][1] is None and res["grads_x_alone"][0] is None, what + ": a gradient nobody asked for"
        assert bits(res["grads_g_alone"][0], res["grads"][0]) and bits(res["grads_x_alone"][1], res["grads"][1]), what + ": one gradient alone has other bits"
    # 16 bits: bitwise the float32 call on the widened tensor, the gate gradient rounded once
    out32, grads32 = (res["out32"], res["grads32"]) if sixteen else (res["out"], res["grads"])
    if sixteen:
        _same(res["out"], out32, what + " 16-bit forward against the widened float32 call")
        if case.family == "kxk":
            _same(res["out32_hist"], out32, what + " widened forward that keeps its levels")
            kept = (case.n if case.contract == "assemble" else case.n - 1) * res["out"].numel()   # (a history of no level is one unwritten element)
            assert bits(res["history"][:kept], res["history32"][:kept]), what + ": 16-bit history against the widened float32 call's"
        assert res["grads"][0].dtype == res["placed"]["g"].dtype and bits(res["grads"][0], grads32[0].to(res["grads"][0].dtype)), \
            what + ": the 16-bit gate gradient is not the float32 one rounded once"
        _same(tuple(res["grads"][1:]), tuple(grads32[1:]), what + " 16-bit backward against the widened float32 call")
    # the float32 results against the float64 statement
    assert bool(ref.isfinite().all()) and all(bool(v.isfinite().all()) for v in ref_grads.values()), what + ": the float64 statement is not finite"
    used["out"] = fraction(out32.cpu().numpy(), ref.numpy(), fwd_bound, what + " out")
    for i, r in enumerate(roles):
        used["d/d" + r] = fraction(grads32[i].cpu().numpy(), ref_grads[r].numpy(), grad_bound, what + " d/d" + r)
    # anchors to the neighbouring entry points
    if "unit_out" in res:
        n, L = case.n, res["out"].numel()
        _same(res["unit_out"], res["norm_out"], what + " one level, conf = 1: cspn2d_forward_kxk_norm")
        assert bits(res["unit_history"][:(n - 1) * L], res["norm_history"][:(n - 1) * L]) and \
            bits(res["unit_history"][(n - 1) * L:n * L].view_as(res["norm_out"]), res["norm_out"]), what + " one level, conf = 1: the history"
        _same(tuple(res["unit_grads"][:2]), tuple(res["norm_grads"]), what + " one level, conf = 1: cspn2d_backward_kxk_norm")
    if "multi_out" in res:
        _same(res["multi_out"], res["out"], what + " C = 1 through cspn3d_forward_norm_multi_*")
        _same(res["multi_grads"], res["grads"], what + " C = 1 through cspn3d_backward_norm_multi_*")
    if "persistent_out" in res:
        _same(res["persistent_out"], res["auto_out"], what + " forward: 'persistent' is what 'auto' runs")
        used["out persistent"] = fraction(res["persistent_out32"].cpu().numpy(), ref.numpy(), fwd_bound, what + " out, persistent")
    if "persistent_grads" in res:
        _same(res["persistent_grads"], res["auto_grads"], what + " backward: 'persistent' is what 'auto' runs")
        for i, r in enumerate(roles):
            used["d/d%s persistent" % r] = fraction(res["persistent_grads32"][i].cpu().numpy(), ref_grads[r].numpy(), grad_bound, what + " persistent d/d" + r)
    for r, v in res["before"].items():
        assert bits(res["placed"][r], v), "%s: the calls wrote input %r" % (what, r)
    return used


# ---- the soak ----
def _paths():
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)


def main(argv):
    """FUZZ_CASES K x K cases, half as many 3D ones and as many head ones of FUZZ_SEED, or the one case whose descriptor is the argument; a case whose
    float32 statement uses more than half of a bound is named and left out (a failure must mean the kernel); stops at the first failure"""
    _paths()
    if len(argv) > 1:
        cases = [eval(argv[1], {"__builtins__": {}}, {"KxK": KxK, "Vol": Vol, "Head": Head})]
    else:
        count, seed = int(os.environ.get("FUZZ_CASES", "60")), int(os.environ.get("FUZZ_SEED", "1"))
        cases = draw("kxk", seed, count) + draw("3d", seed, count // 2) + draw("head", seed, count)
    ran = 0
    for case in cases:
        try:
            cost = max(statement_fractions(case))
        except AssertionError as e:   # past a whole bound
            print("inadmissible %r: %s" % (case, e), flush=True)
            continue
        if cost > 0.5:
            print("inadmissible %r: the float32 statement uses %.3g of a bound" % (case, cost), flush=True)
            continue
        try:
            used = check(case)
        except Exception as e:   # an assertion, an engine error or a HIP error: nothing more runs
            print("FAILED %r\n%s: %s" % (case, type(e).__name__, e), flush=True)
            return 1
        ran += 1
        print("ok %.3f (float32 statement %.3f) %r" % (max(used.values()), cost, case), flush=True)
    print("FUZZ OK: %d cases, %d inadmissible left out" % (ran, len(cases) - ran))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
