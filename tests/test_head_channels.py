"""The four guidance-head paths past one chunk of 64 channels, between guard bands and through a stale arena (tests/memguard.py, the machinery of
tests/test_memory_hygiene.py).  The backwards walk the input channels 64 at a time on the host, every chunk's launches followed by a
reduce launch over ONE shared buffer of partial blocks; the packed weight records and the workspaces grow with C.  tests/test_memory_hygiene.py's
table stops at C = 64, one chunk.  Here: C = 97 (A, C: a second chunk of two column blocks) and C = 129 (B, D: a third chunk of one channel), a
narrowed odd output, and C = 129 -> 65 -> 129 through one arena that is never refilled.  The values themselves are held to the float64 statement
by the seeded draws of tests/test_fuzz_statements.py (family 'head')."""
import contextlib
import functools

import pytest
import torch

import memguard
import test_memory_hygiene as hygiene
from cspn_amd import train_utils as T

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SHAPE = (2, 5, 33, 9, 65)          # B, h, w -> H x W: narrowed (H < 2 h), odd W, w one past a 32-column segment
# path -> (_HEAD_PATHS key, guidance planes, dtype of x, C of the guarded case)
PATHS = {"A": ("f32", 8, F32, 97), "B": ("kxk_f32", 48, F32, 129), "C": ("kxk_g16", 24, BF16, 97), "D": ("g16", 8, F16, 129)}


def _guidance_dtype(path):
    return F32 if path == "D" else None


def _inputs(path, C, seed):
    """x (its path's dtype), the float32 master weights, dL/dguidance in the path's guidance dtype, dL/dblur float32, on the GPU"""
    _, P, dt, _ = PATHS[path]
    B, h, w, H, W = SHAPE
    gen = torch.Generator().manual_seed(seed)
    s = 3.0 * C ** 0.5
    x = torch.randn(B, C, h, w, generator=gen).cuda().to(dt)
    wg, wb = (torch.randn(P, C, 3, 3, generator=gen) / s).cuda(), (torch.randn(1, C, 3, 3, generator=gen) / s).cuda()
    gg = torch.randn(B, P, H, W, generator=gen).cuda().to(dt if path == "C" else F32)
    gb = torch.randn(B, 1, H, W, generator=gen).cuda()
    return x, wg, wb, gg, gb


def _call(path):
    gd = _guidance_dtype(path)
    H, W = SHAPE[3:]

    def call(x, wg, wb, gg, gb):
        return T.guidance_heads(x, wg, wb, H, W, guidance_dtype=gd) + T.guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=gd)
    return call


def _plane(P):
    B, _, _, H, W = SHAPE
    return 4 * B * P * H * W


HYGIENE = {}
for _path, (_key, _P, _dt, _C) in PATHS.items():
    _name = "heads-%s-C%d-%d-%s" % (_path, _C, _P, str(_dt).split(".")[1])
    HYGIENE[_name] = hygiene.Case(_name, ("guidance_heads", "guidance_heads_backward"),
                                  "_HEAD_PATHS[%r], forward and backward, %d chunks of 64 channels" % (_key, (_C + 63) // 64), _plane(_P),
                                  functools.lru_cache(maxsize=None)(functools.partial(_inputs, _path, _C, 700 + _C + _P)), _call(_path), lambda: None,
                                  "test_fuzz_statements.py (family 'head', path %s)" % _path, False, None, None)


def test_the_guarded_cases_stay_out_of_the_shared_table_and_pass_one_chunk():
    assert not set(HYGIENE) & set(hygiene.CASES) and {c.plane > 0 for c in HYGIENE.values()} == {True}
    assert sorted(PATHS) == ["A", "B", "C", "D"] and all(C > 64 for _, _, _, C in PATHS.values())
    for path, (key, P, dt, _) in PATHS.items():
        assert T._head_path(torch.empty(1, 1, 1, 1, dtype=dt), torch.empty(P, 1, 3, 3), None, P, _guidance_dtype(path)) is T._HEAD_PATHS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYGIENE))
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_every_path_past_one_chunk_between_guard_bands(name, poison):
    """the workspace and the outputs lie between guard bands and are poisoned before the calls: finite outputs, bitwise the unguarded run's, intact
    bands, unchanged inputs.  A packed-record or partial-block region sized for fewer channels than it holds shows here"""
    c = HYGIENE[name]
    inputs = c.build()
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, c.call, inputs, "cuda", c.plane)
    assert len(session.workspaces) == 2 and len(session.guards) > len(session.workspaces)
    assert len(outs) == 5
    for o in outs:
        assert o is not None and bool(torch.isfinite(o.float()).all()), "poison reached an output"
    memguard.assert_same_outputs(outs, hygiene._clean(c), "poison %r" % poison)


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(PATHS))
def test_stale_arena_three_chunks_two_chunks_three_chunks(path):
    """C = 129, then C = 65, then C = 129 again through one arena that is never refilled: a chunk that reads the chunk before it, or a narrower
    call that reads what a wider one left in the partial blocks, gives other bits than the clean run"""
    call = _call(path)
    steps = [("%s C = %d" % (path, C), call, _inputs(path, C, 800 + C + i)) for i, C in enumerate((129, 65, 129))]
    hygiene._run_sequence(steps, _plane(PATHS[path][1]))
