"""A seeded fuzz of the K x K engine's four contracts and of the 3D normalising / masked modes against the float64 statements of their own test
files (tests/fuzzcases.py draws, places, runs and checks).  The bounds are the project's, none is defined here.
CPU: the draw and the inputs are reproducible; the list of the committed seed reaches every stratum below; every reference is finite, and the
     same statement evaluated in float32 on the CPU stays within HALF of every bound, so that a failure on the GPU means the kernel.
GPU: one test per drawn case, then one that counts them."""
import pytest

import fuzzcases
from fuzzcases import CONTRACTS, DTYPES, KERNELS, NEEDS, ROLES, TILE_H, TILE_W, steps_of, takes_persistent

SEED = 1   # (most seeds reach every stratum; 14, 20 and 21 are the first that do not)
COUNTS = {"kxk": 60, "3d": 30}
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


STRATA = {"kxk": _kxk_strata(), "3d": _3d_strata()}


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


def test_the_inputs_are_reproducible():
    import torch
    for family in fuzzcases.FAMILIES:
        for c in CASES[family][:6]:
            a, b = fuzzcases.inputs(c), fuzzcases.inputs(c)
            assert a.keys() == b.keys()
            for r in a:
                assert (a[r] is None and b[r] is None) or (not a[r].is_cuda and a[r].dtype == b[r].dtype and torch.equal(a[r], b[r])), (c, r)
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
    """the float64 reference is finite, and the float32 statement on the CPU lies within half of every bound the GPU result is held to"""
    worst = {"forward": (0.0, None), "gradient": (0.0, None)}
    for c in CASES[family]:
        ref, grads = fuzzcases.reference(c)
        assert bool(ref.isfinite().all()) and all(bool(g.isfinite().all()) for g in grads.values()), "%r: the float64 statement is not finite" % (c,)
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
    assert len(_RAN) == len(IDS) == 90, "%d of %d cases ran to their end; missing %s" % (len(_RAN), len(IDS), sorted(set(IDS) - _RAN))
