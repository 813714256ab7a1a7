"""A seeded fuzz of the K x K engine's four contracts, of the 3D normalising / masked modes and of the four guidance-head paths (past the 64-channel
chunks of their backwards) against the float64 statements of their own test files (tests/fuzzcases.py draws, places, runs and checks).  The bounds are the project's, none is defined here.
CPU: the draw and the inputs are reproducible; the list of the committed seed reaches every stratum below; every reference is finite, and the
     same statement evaluated in float32 on the CPU stays within HALF of every bound, so that a failure on the GPU means the kernel.
GPU: one test per drawn case, then one that counts them."""
import os
import re

import pytest

import fuzzcases
from fuzzcases import (CONTRACTS, DTYPES, HEAD_CLASSES, HEAD_DTYPES, HEAD_DW, HEAD_NEEDS, HEAD_NORMS, HEAD_PATHS, HEAD_PLANES, HEAD_ROLES, KERNELS, NEEDS, ROLES,
                       TILE_H, TILE_W, chunk_class, head_out_size, head_tiles, offsets_of, steps_of, takes_persistent)

SEED = 1   # (most seeds reach every stratum; 14, 20 and 21 are the first that do not; of the head family 2, 13 and 17, which have no case of W = 1)
COUNTS = {"kxk": 60, "3d": 30, "head": 64}
CASES = {family: fuzzcases.draw(family, SEED, count) for family, count in COUNTS.items()}
IDS = [(family, i) for family in fuzzcases.FAMILIES for i in range(COUNTS[family])]


def _grid(c):
    return (c.W + TILE_W - 1) // TILE_W, (c.H + TILE_H - 1) // TILE_H   # tile columns, tile rows


def _kxk_strata():
    s = []
    for contract in CONTRACTS:
        mine = lambda c, contract=contract: c.contract == contract   # noqa: E731
        for K in KERNELS[contract]:
            s.append(("%s K=%d" % (contract, K), lambda c, mine=mine, K=K: mine(c) and c.K == K))
        for dtype in DTYPES:
            s.append(("%s %s" % (contract, dtype), lambda c, mine=mine, dtype=dtype: mine(c) and c.dtype == dtype))
        for role in ROLES[contract]:
            s.append(("%s W %% 4 = 0, %s alone offset" % (contract, role), lambda c, mine=mine, role=role: mine(c) and c.W % 4 == 0 and c.offset == role))
        for need in NEEDS[contract]:
            s.append(("%s need=%s" % (contract, need), lambda c, mine=mine, need=need: mine(c) and c.need == need))
        if contract != "none":
            s.append(("%s >= 3 x 2 tiles" % contract, lambda c, mine=mine: mine(c) and _grid(c)[0] >= 3 and _grid(c)[1] >= 2))
            s.append(("%s >= 2 x 3 tiles" % contract, lambda c, mine=mine: mine(c) and _grid(c)[0] >= 2 and _grid(c)[1] >= 3))
    for r in range(4):
        s.append(("W %% 4 = %d" % r, lambda c, r=r: c.W % 4 == r))
    s += [("W < K", lambda c: c.W < c.K), ("H < K", lambda c: c.H < c.K)]
    s += [("W = %d" % w, lambda c, w=w: c.W == w) for w in (TILE_W, 2 * TILE_W)] + [("H = %d" % h, lambda c, h=h: c.H == h) for h in (TILE_H, 2 * TILE_H)]
    s += [("mask %s, C > 1" % m, lambda c, m=m: c.contract in ("norm", "assemble") and c.mask == m and c.C > 1) for m in fuzzcases.MASKS2D]
    s += [("B = 1", lambda c: c.B == 1), ("B = 3", lambda c: c.B == 3), ("C = 1", lambda c: c.C == 1), ("C = 4", lambda c: c.C == 4)]
    asm = lambda c: c.contract == "assemble"   # noqa: E731
    s += [("assemble collects level 0", lambda c: asm(c) and steps_of(c)[0] == 0), ("assemble T = n + 1", lambda c: asm(c) and len(steps_of(c)) == c.n + 1),
          ("assemble T = 1", lambda c: asm(c) and len(steps_of(c)) == 1), ("assemble n = 1", lambda c: asm(c) and c.n == 1)]
    return s


def _3d_strata():
    partial = lambda c: c.D % 8 != 0 or c.H % 8 != 0 or c.W % 64 != 0   # noqa: E731   (the persistent kernel's tile is 8 x 8 x 64)
    s = [("W % 4 != 0", lambda c: c.W % 4 != 0), ("W % 4 = 0, W < 64", lambda c: c.W % 4 == 0 and c.W < 64),
         ("persistent both ways: W % 4 = 0, W >= 64, n >= 3, partial tiles, nothing offset", lambda c: takes_persistent(c) and c.n >= 3 and partial(c)),
         ("D = 1", lambda c: c.D == 1), ("H = 1", lambda c: c.H == 1), ("C = 1", lambda c: c.C == 1), ("C > 1", lambda c: c.C > 1),
         ("guidance alone offset", lambda c: c.offset == "g"), ("feat alone offset", lambda c: c.offset == "x")]
    s += [("mask %s" % m, lambda c, m=m: c.mask == m) for m in fuzzcases.MASKS3D]
    s += [("norm %s" % n, lambda c, n=n: c.norm == n) for n in fuzzcases.NORMS]
    s += [(d, lambda c, d=d: c.dtype == d) for d in DTYPES]
    return s


def _head_strata():
    s = []
    W = lambda c: head_out_size(c)[1]   # noqa: E731
    for path in HEAD_PATHS:
        mine = lambda c, path=path: c.path == path   # noqa: E731
        for k, name in enumerate(HEAD_CLASSES):
            s.append(("%s %s" % (path, name), lambda c, mine=mine, k=k: mine(c) and chunk_class(c.C) == k))
        for planes in HEAD_PLANES[path]:
            s.append(("%s %d planes" % (path, planes), lambda c, mine=mine, planes=planes: mine(c) and c.planes == planes))
        for dtype in HEAD_DTYPES[path]:
            s.append(("%s %s" % (path, dtype), lambda c, mine=mine, dtype=dtype: mine(c) and c.dtype == dtype))
        for role in HEAD_ROLES:
            s.append(("%s W %% 4 = 0, exact 2x, %s alone offset" % (path, role),
                      lambda c, mine=mine, role=role: mine(c) and c.offset == role and c.oh == 0 and (2 * c.w) % 4 == 0))
        s.append(("%s more dL/dW tiles than waves at C > 64" % path, lambda c, mine=mine: mine(c) and c.C > 64 and "w" in c.need and head_tiles(c) > HEAD_DW[c.path][1]))
        # the seven `c0 += 64` loops of cspn_amd/csrc: dL/dW on every path, dL/dx on B, C and D (A's dL/dx kernel walks the channels itself)
        s.append(("%s dL/dW asked for at C > 64" % path, lambda c, mine=mine: mine(c) and c.C > 64 and "w" in c.need))
        s.append(("%s dL/dW asked for at C > 128: three chunks" % path, lambda c, mine=mine: mine(c) and c.C > 128 and "w" in c.need))
        if path != "A":
            s.append(("%s dL/dx asked for at C > 64" % path, lambda c, mine=mine: mine(c) and c.C > 64 and "x" in c.need))
            s.append(("%s dL/dx asked for at C > 128: three chunks" % path, lambda c, mine=mine: mine(c) and c.C > 128 and "x" in c.need))
        if path in "CD":
            s.append(("%s weights of x's dtype" % path, lambda c, mine=mine: mine(c) and c.w16 == 1))
    s += [("A norm %s" % n, lambda c, n=n: c.path == "A" and c.norm == n) for n in HEAD_NORMS]
    s += [("need=%s" % n, lambda c, n=n: c.need == n) for n in HEAD_NEEDS]
    s += [("a blur head", lambda c: c.blur == 1), ("no blur head", lambda c: c.blur == 0)]
    s += [("exact 2x", lambda c: c.oh == 0), ("narrowed", lambda c: c.oh != 0 and (c.oh < 2 * c.h or c.ow < 2 * c.w)), ("odd W", lambda c: W(c) % 2 == 1),
          ("odd H", lambda c: head_out_size(c)[0] % 2 == 1), ("W % 4 = 0", lambda c: W(c) % 4 == 0), ("W % 4 != 0", lambda c: W(c) % 4 != 0),
          ("w = 1", lambda c: c.w == 1), ("W = 1", lambda c: W(c) == 1), ("h = 1", lambda c: c.h == 1), ("w < 32", lambda c: c.w < 32), ("w > 32", lambda c: c.w > 32),
          ("A w < 63", lambda c: c.path == "A" and c.w < 63), ("A w > 63", lambda c: c.path == "A" and c.w > 63), ("C % 2 = 1", lambda c: c.C % 2 == 1),
          ("nothing offset", lambda c: c.offset == "")]
    return s


STRATA = {"kxk": _kxk_strata(), "3d": _3d_strata(), "head": _head_strata()}


# ---- CPU ----
def test_the_draw_is_reproducible_and_obeys_its_rules():
    for family, count in COUNTS.items():
        again = fuzzcases.draw(family, SEED, count)
        assert again == CASES[family] and len(again) == count
        assert fuzzcases.draw(family, SEED + 1, count) != again
    for c in CASES["kxk"]:
        assert c.contract == CONTRACTS[c.index % 4] and c.K in KERNELS[c.contract] and c.dtype in DTYPES and c.need in NEEDS[c.contract]
        assert 1 <= c.B <= 3 and 1 <= c.C <= 4 and c.W in fuzzcases.KXK_W and 1 <= c.n <= fuzzcases.N_MAX
        assert c.B * c.C * c.H * c.W <= fuzzcases.KXK_ELEMENTS and any(c.H == h >> k for h in fuzzcases.KXK_H for k in range(6))
        assert c.contract == "none" or c.H * c.W > (1 if c.contract == "absnorm" else 2)
        assert set(c.offset) <= set(ROLES[c.contract]) and ("s" not in c.offset or c.mask != "none")
        if c.contract == "assemble":
            st = steps_of(c)
            assert 1 <= len(st) <= fuzzcases.T_MAX and st[0] >= 0 and st[-1] == c.n and all(a < b for a, b in zip(st, st[1:]))
        else:
            assert c.steps == ""
    assert [sum(c.contract == k for c in CASES["kxk"]) for k in CONTRACTS] == [15] * 4
    for c in CASES["3d"]:
        assert c.norm in fuzzcases.NORMS and c.mask in fuzzcases.MASKS3D and c.dtype in DTYPES and c.algo in ("auto", "stepwise")
        assert 1 <= c.B <= 2 and 1 <= c.C <= 4 and c.W in fuzzcases.VOL_W and 1 <= c.n <= fuzzcases.N_MAX
        assert c.B * c.C * c.D * c.H * c.W <= fuzzcases.VOL_ELEMENTS and c.D * c.H * c.W > 2
        assert set(c.offset) <= set(ROLES["3d"]) and ("s" not in c.offset or c.mask != "nomask")
    for c in CASES["head"]:
        slot = c.index // 4
        assert c.path == HEAD_PATHS[c.index % 4] and c.planes in HEAD_PLANES[c.path] and c.dtype in HEAD_DTYPES[c.path] and c.need in HEAD_NEEDS
        assert c.norm in (HEAD_NORMS if c.path == "A" else ("",)) and c.w16 in ((0, 1) if c.path in "CD" else (0,)) and c.blur == int(slot % 4 != 3)
        assert set(offsets_of(c)) <= set(HEAD_ROLES if c.blur else [r for r in HEAD_ROLES if not r.endswith("blur")])
        assert (c.oh, c.ow) == (0, 0) or (max(1, 2 * c.h - 3) <= c.oh <= 2 * c.h and max(1, 2 * c.w - 3) <= c.ow <= 2 * c.w)
        if slot == 5:      # more tiles than waves, by the smallest h: one row of tiles less no longer has
            px, waves = HEAD_DW[c.path]
            assert (c.B, c.C, c.w) == fuzzcases.HEAD_MANY[c.path] and c.C > 64 and (c.oh, c.offset, c.need) == (0, "", "xw")
            assert head_tiles(c) > waves >= head_tiles(c) - c.B * ((c.w + px - 1) // px)
        else:
            assert 1 <= c.B <= 3 and c.C in fuzzcases.HEAD_C and c.w in fuzzcases.HEAD_W and c.B * c.C * c.h * c.w <= fuzzcases.HEAD_ELEMENTS
            assert any(c.h == h >> k for h in range(1, fuzzcases.HEAD_H_MAX + 1) for k in range(4)) and c.h >= 1
        if slot < len(HEAD_ROLES):
            assert c.offset == HEAD_ROLES[slot] and c.oh == 0 and c.w % 2 == 0 and not (c.w16 and c.offset.startswith("weight"))
    assert [sum(c.path == p for c in CASES["head"]) for p in HEAD_PATHS] == [16] * 4
    for p in HEAD_PATHS:   # 15 deals of a 14-card deck: every C of the list, so every chunk class, on every path
        assert {c.C for c in CASES["head"] if c.path == p and c.index // 4 != 5} == set(fuzzcases.HEAD_C)


def test_the_head_draw_has_the_host_codes_tile_and_wave_counts():
    """HEAD_DW against cspn_amd/csrc: the slot 'more tiles than waves' is sized by them"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cspn_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()   # noqa: E731
    const = lambda text, name: int(re.search(r"constexpr int (?:\w+ = \w+, )*%s = (\d+)[,;]" % name, text).group(1))   # noqa: E731
    a, b, common, g16 = read("cspn_head_backward.hip"), read("cspn_head_kxk.hip"), read("cspn_head_kxk_common.h"), read("cspn_head_g16_common.h")
    assert "nwave = tiles < 4 * DW_MAX_WG ? tiles : 4 * DW_MAX_WG" in common and "nwave = tiles < DW_MAX_WAVES ? tiles : DW_MAX_WAVES" in a
    assert "DW_TILE = 2 * DW_PX" in b and "DwGeo G(B, h, w, H, W, O, DW_TILE)" in b
    waves = 4 * const(common, "DW_MAX_WG")
    assert HEAD_DW == {"A": (const(a, "W2_TP"), const(a, "DW_MAX_WAVES")), "B": (2 * const(b, "DW_PX"), waves), "C": (const(g16, "DW_TILE"), waves),
                       "D": (const(g16, "DW_TILE"), waves)}
    loops = sum(read(n).count("c0 += 64") for n in ("cspn_head_backward.hip", "cspn_head_kxk.hip", "cspn_head_kxk_g16.hip", "cspn_head_g16.hip"))
    assert loops == 7      # the loops the strata 'asked for at C > 64' are written against: dL/dW on A, dL/dx and dL/dW on B, C and D


def test_the_inputs_are_reproducible():
    import torch
    for family in fuzzcases.FAMILIES:
        for c in CASES[family][:6]:
            a, b = fuzzcases.inputs(c), fuzzcases.inputs(c)
            assert a.keys() == b.keys()
            for r in a:
                assert (a[r] is None and b[r] is None) or (not a[r].is_cuda and a[r].dtype == b[r].dtype and torch.equal(a[r], b[r])), (c, r)
            if family == "head":
                g16 = "torch." + c.dtype if c.path == "C" else "torch.float32"
                assert str(a["x"].dtype) == "torch." + c.dtype and str(a["grad_guidance"].dtype) == g16
                assert str(a["weight_guidance"].dtype) == ("torch." + c.dtype if c.w16 else "torch.float32")
                assert (a["weight_blur"] is None) == (a["grad_blur"] is None) == (not c.blur)
                continue
            assert str(a["g"].dtype) == "torch." + c.dtype and a["x"].dtype == a["o"].dtype == torch.float32


@pytest.mark.parametrize("family", fuzzcases.FAMILIES)
def test_the_committed_seed_reaches_every_stratum(family):
    missing = []
    print("\n%s, seed %d, %d cases" % (family, SEED, COUNTS[family]))
    for name, hit in STRATA[family]:
        where = [c.index for c in CASES[family] if hit(c)]
        print("  %-84s %2d  %s" % (name, len(where), where[:8]))
        if not where:
            missing.append(name)
    assert not missing, "seed %d leaves out: %s" % (SEED, "; ".join(missing))


@pytest.mark.parametrize("family", fuzzcases.FAMILIES)
def test_every_case_is_admissible(family):
    """the float64 reference is finite, and the float32 statement on the CPU lies within half of every bound the GPU result is held to (a head result
    stored in 16 bits: the unrounded float32 statement within half of the 1e-5 max |ref| term alone, fuzzcases._head_statement_fractions)"""
    worst = {"forward": (0.0, None), "gradient": (0.0, None)}
    for c in CASES[family]:
        assert fuzzcases.finite(fuzzcases.reference(c)), "%r: the float64 statement is not finite" % (c,)
        for kind, f in zip(("forward", "gradient"), fuzzcases.statement_fractions(c)):
            assert f <= 0.5, "%r: the float32 statement uses %.3g of the %s bound" % (c, f, kind)
            if f > worst[kind][0]:
                worst[kind] = (f, c.index)
    print("\n%s: the float32 statement's worst fraction of the forward bound %.3g (case %s), of the gradient bound %.3g (case %s)"
          % (family, worst["forward"][0], worst["forward"][1], worst["gradient"][0], worst["gradient"][1]))


# ---- GPU ----
_RAN = set()


@pytest.mark.gpu
@pytest.mark.parametrize("family,index", IDS)
def test_case(family, index):
    case = CASES[family][index]
    try:
        used = fuzzcases.check(case)
    except AssertionError as e:
        raise AssertionError("%r\n%s" % (case, e)) from e
    print("%r\n  fractions of the bounds: %s" % (case, ", ".join("%s %.3g" % kv for kv in sorted(used.items()))))
    _RAN.add((family, index))


@pytest.mark.gpu
def test_every_drawn_case_ran():
    assert len(_RAN) == len(IDS) == 154, "%d of %d cases ran to their end; missing %s" % (len(_RAN), len(IDS), sorted(set(IDS) - _RAN))
