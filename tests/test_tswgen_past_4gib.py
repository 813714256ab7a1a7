"""Both generated ring loops (tools/tswgen/kernel.py: 8 waves x 4 rows, kernel4.py: 12 waves x 3 rows) in the CPU emulator at guidance
offsets of 4 GiB and more: dword 1 of the row descriptors (cspn2d_tsw_desc.h) is non-zero and the s_add_u32 / s_addc_u32 chains behind
it carry.  A batch that large is not held: tools/tswgen/run_emu.py `window` runs the band groups that lie wholly in a few of its images,
with the large batch's descriptors, on tensors at virtual addresses of which only those images (and image 0) exist -- an address that
lost its high dword or a carry is an EmuError (or reads NaNs), not a silent read.  Every case is checked against the oracle."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.tswgen import kernel as K  # noqa: E402
from tools.tswgen import plan as P  # noqa: E402
from tools.tswgen.run_emu import run_case  # noqa: E402
from tools.tswgen.run_emu4 import run_case as run_case4  # noqa: E402

LINE = 1 << 32
H = 21
# byte 2^32 of the guidance tensor [B][8][H][W] lies in plane 0 of image B_LINE[W], in row Y_LINE[W]: a stream over that image's rows
# has descriptors on both sides of the line (dword 0 wraps, dword 1 goes from 0 to 1 inside the stream)
B_LINE = {304: LINE // (32 * H * 304), 256: LINE // (32 * H * 256)}
Y_LINE = {W: (LINE - b * 32 * H * W) // (4 * W) for W, b in B_LINE.items()}
SHARE = 24   # image rows per band group of the large batch's plan: a stream the emulator runs in seconds


def big_plan(W, b0, nimg, straddle):
    """-> (B_total, n_wg): a batch whose plan (band groups of about SHARE rows) has a group wholly inside the images b0 .. b0 + nimg - 1 that
    starts mid-image; straddle: and owns the row of image b0 that holds byte 2^32 of the guidance"""
    nb = len(P.plan_bands(W, 24))
    for B_total in range(b0 + nimg, b0 + nimg + 64):
        total = B_total * H
        ng = total // SHARE
        for G in range(b0 * H * ng // total, (b0 + nimg) * H * ng // total + 1):
            r0, r1 = total * G // ng, total * (G + 1) // ng
            if r0 < b0 * H or r1 > (b0 + nimg) * H or r0 % H == 0:
                continue
            if straddle and not r0 + 2 <= b0 * H + Y_LINE[W] < r1 - 2:
                continue
            return B_total, ng * nb
    raise AssertionError("no such plan")


def test_the_shapes_are_where_the_docstring_says():
    assert (B_LINE, Y_LINE) == ({304: 21024, 256: 24966}, {304: 13, 256: 16})
    for W, b in B_LINE.items():
        at = 32 * H * W * b + 4 * W * Y_LINE[W]   # first byte of that row in plane 0
        assert at <= LINE < at + 4 * W
        assert (b + 8) * H * W <= 0x7fffffff // 9   # (what check_index32(B H W, 9) of cspn_abi.cpp accepts)


@pytest.mark.parametrize("W,b0,straddle", [(304, B_LINE[304], True), (256, B_LINE[256] + 1, False)])
def test_numpy_plan_descriptors_reassemble_the_64_bit_guidance_offset(W, b0, straddle):
    """tools/tswgen/plan.py for such a batch: d[0] | d[1] << 32 of every active descriptor is the byte offset of (image, plane 0, y, p0)
    in the guidance tensor, recomputed here from the stream in Python integers; d[2] the same in a 1-channel tensor"""
    B_total, n_wg = big_plan(W, b0, 2, straddle)
    wgs, hdr, tab, rows = P.build_plan_window(B_total, H, W, 24, n_wg, b0, 2)
    bands = P.plan_bands(W, 24)
    assert len(wgs) == len(bands) and rows.any()
    highs = set()
    for i, g in enumerate(wgs):
        segs = P.share_segments(B_total, H, W, 24, bands, g, n_wg)
        stream = P.stream_of(segs)
        assert hdr[i, 0] == len(stream)
        for q, r in enumerate(stream):
            d = [int(x) for x in tab[i, K.PADF + q]]
            if r is None:
                assert d == [0, 0, 0, 0]
                continue
            b, bi = segs[r[0]][0], segs[r[0]][1]
            goff = 4 * (b * 8 * H * W + r[1] * W + bands[bi][0])
            assert d[0] | d[1] << 32 == goff and d[3] & 1
            assert d[2] == 4 * (b * H * W + r[1] * W + bands[bi][0]) < LINE
            highs.add(d[1])
    assert highs == ({0, 1} if straddle else {1})


def check(res, tol):
    err, nanmis, out, ref, rows = res
    assert nanmis == 0
    assert err <= tol, err
    assert rows.sum() >= SHARE - 1


def test_ring8x4_stream_that_straddles_the_line():
    """8sum, no mask, two bands: the group owns rows on both sides of byte 2^32 (dword 0 of its descriptors wraps inside the stream)"""
    os.chdir(ROOT)
    W, b0 = 304, B_LINE[304]
    B_total, n_wg = big_plan(W, b0, 2, True)
    res = run_case(2, H, W, n_wg, 0, False, seed=1, verbose=False, window=(B_total, b0))
    check(res, 1e-4)
    assert res[4][0, Y_LINE[W]]


def test_ring8x4_with_mask_past_the_line():
    """8sum_abs with a mask and a NaN patch; every row the group streams starts past the line"""
    os.chdir(ROOT)
    W, b0 = 304, B_LINE[304] + 1
    B_total, n_wg = big_plan(W, b0, 2, False)
    res = run_case(2, H, W, n_wg, 1, True, seed=2, zero_patch=True, verbose=False, window=(B_total, b0))
    check(res, 1e-4)
    assert np.isnan(res[3]).any()


def test_sited8_layout_rebuilds_the_high_part_from_dword_2():
    """cfg s8 (32 bytes per pixel): the row starts at 8 x its 1-channel byte offset, the high part is dword 2 >> 29 (non-zero here)"""
    os.chdir(ROOT)
    W, b0 = 256, B_LINE[256]
    B_total, n_wg = big_plan(W, b0, 2, True)
    assert 4 * b0 * H * W >> 29 == 0 and 4 * (b0 + 1) * H * W >> 29 == 1   # both values of the high part in the stream
    check(run_case(2, H, W, n_wg, 0, True, seed=3, verbose=False, s8=True, window=(B_total, b0)), 1e-4)


def test_history_variant_past_the_line():
    """cfg hist: checkpoints and folded planes (their planes B_total images apart: S_HSTRIDE is the large batch's) next to guidance reads
    past the line"""
    os.chdir(ROOT)
    W, b0 = 256, B_LINE[256] + 1
    B_total, n_wg = big_plan(W, b0, 2, False)
    check(run_case(2, H, W, n_wg, 0, True, seed=4, verbose=False, hist=True, hist_every=K.HIST_EVERY, window=(B_total, b0)), 1e-4)


def test_prefetch_with_its_clamp_at_zero():
    """cfg pf with S_GLAST = 0, what cspn2d_tsw.hip passes for a guidance tensor of 4 GiB or more: the 32-bit sum is clamped to 0, every
    touch lands on the first rows of the tensor (image 0 exists in the emulated memory; anywhere else would be an EmuError)"""
    os.chdir(ROOT)
    W, b0 = 256, B_LINE[256]
    B_total, n_wg = big_plan(W, b0, 2, True)
    assert 32 * H * W * B_total >= LINE
    check(run_case(2, H, W, n_wg, 0, False, seed=5, verbose=False, cfg_extra=dict(pf=True), window=(B_total, b0)), 1e-4)


def test_ring12x3_stream_that_straddles_the_line():
    """the 12 x 3 ring (LDS-DMA rows from per-plane bases + the descriptor's 64-bit offset), 8sum with a mask, two bands, rows on both sides
    of the line"""
    os.chdir(ROOT)
    W, b0 = 304, B_LINE[304]
    B_total, n_wg = big_plan(W, b0, 2, True)
    res = run_case4(2, H, W, n_wg, 0, True, seed=6, verbose=False, window=(B_total, b0))
    check(res, 1e-5)
    assert res[4][0, Y_LINE[W]]

