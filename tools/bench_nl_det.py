"""The run-to-run bitwise backward of non-local propagation (cspn2d_backward_nl_det: an inverted index per call, an order-independent gathered
sum) beside the scatter backward (cspn2d_backward_nl: float atomics), in the setup of tools/bench_nl.py: KITTI x 8 (B 8, 1 x 304 x 1216), n_iter 18,
C 1, K 3, affinities randn * 0.2, ~500 measured points per image, `random` and `smooth` offsets.  Writes profiles/nl_det.md.
Measured, the two variants taking turns block by block in the same run: the backward alone (all three gradients, on a kept history), the training
step (the forward that keeps its history, then the backward), peak memory of both, and for the deterministic backward the index build apart from the
sweeps: with T(n) the time of the grad_x-only backward at n steps (the index and n gathered sweeps, no gate gradient), a sweep is
(T(18) - T(1)) / 17 and the build T(1) minus one sweep.  No ratio is a pass condition: the file reports whichever way it falls.
    python tools/bench_nl_det.py [--reps 3] [--blocks 3] [--md profiles/nl_det.md] [--json out.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_nl import B, C, H, KK, N_ITER, W, blocks_of, fmt, peak_mib, rel, stats  # noqa: E402

# what the compiler reports for cspn_amd/csrc/cspn2d_nl_det.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, -S for the
# disassembly): not measured by this tool, recorded here so that the profile has one source
BUILD_REPORT = """\
| kernel | VGPRs | AGPRs | scratch | LDS (bytes) | occupancy (waves / SIMD) |
|---|---|---|---|---|---|
| `nl_index_taps<3, count>` (one source pixel a lane; integer atomics on the counts) | 34 | 0 | 0 | 0 | 8 |
| `nl_index_taps<3, fill>` (integer atomic cursor, one 8-byte store an entry) | 28 | 0 | 0 | 0 | 8 |
| `nl_scan_tiles` (2048 counts a workgroup; the worklist) | 16 | 0 | 0 | 1024 | 8 |
| `nl_scan_sums` (one workgroup) | 18 | 0 | 0 | 1024 | 8 |
| `nl_scan_add` | 6 | 0 | 0 | 0 | 8 |
| `nl_gather_step<propagation>` (one destination a lane; a wave's terms staged in 12 KB of LDS, two passes over them) | 68 | 0 | 0 | 49152 | 3 |
| `nl_gather_step<sampling>` | 52 | 0 | 0 | 49152 | 3 |
| `nl_gather_long<propagation>` (one wave a worklist entry) | 48 | 0 | 0 | 0 | 8 |
| `nl_gather_long<sampling>` | 42 | 0 | 0 | 0 | 8 |

No kernel uses scratch or AGPRs.  The atomics, read once in the unit's disassembly: 72 `global_atomic_add` (the 32-bit integer add: the counts;
the cursors and the worklist counter, which return the old value, `sc0`), and 0 occurrences of `global_atomic_add_f32`, `ds_add_f32`,
`ds_add_rtn_f32`, `pk_add`, `cmpswap` or `cmpst`: the deterministic path holds no float atomic, on global memory or on LDS.

The gathered sweep first walked each lane's list straight from global memory: the 64 loads of a wave instruction then fall into 64 cache
lines, although the wave's 64 lists are one contiguous range of the entries.  Measured once at this shape in that form (ms): a sweep 2.90 with
the `random` offsets and 2.50 with `smooth`, the whole backward 57.9 / 49.7, the training step 60.3 / 52.3.  The figures above are with the
wave's terms formed by coalesced loads and staged in LDS."""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nl_det.md"))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cspn_amd import _lib
    from cspn_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_nl_det.py measures on the GPU; none found")
    gen = torch.Generator(device="cuda").manual_seed(18)   # the draws of tools/bench_nl.py
    aff = torch.randn(B, KK, H, W, device="cuda", generator=gen) * 0.2
    draw = torch.randn(B, 2 * KK, H, W, device="cuda", generator=gen) * 1.5
    low = torch.nn.functional.avg_pool2d(draw, 15, 1, 7)
    fields = {"random": draw, "smooth": low * (draw.std() / low.std())}
    x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
    s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 500 / (H * W)).float() * (x[:, :1] * 0.5 + 0.1)
    go = torch.randn(B, C, H, W, device="cuda", generator=gen)
    backward = {"scatter": F.cspn2d_backward_nl, "deterministic": F.cspn2d_backward_nl_det}
    ws = {"scatter": _lib.symbol("cspn2d_backward_nl_workspace_bytes")(B, C, H, W, 3, N_ITER, 1),
          "deterministic": _lib.symbol("cspn2d_backward_nl_det_workspace_bytes")(B, C, H, W, 3, N_ITER, 1)}
    rows = []
    for name, off in fields.items():
        off = off.contiguous()
        row = dict(shape="kitti_x8", B=B, C=C, H=H, W=W, n_iter=N_ITER, offsets=name, offset_std=round(float(off.std()), 3),
                   workspace_mib={k: round(v / 2 ** 20, 1) for k, v in ws.items()})
        _, hist = F.cspn2d_forward_nl(aff, off, x, s, N_ITER, return_history=True)
        grads = {}

        def bwd(k):
            def f():
                grads[k] = backward[k](aff, off, x, s, go, N_ITER, history=hist)
            return f

        def train(k):
            def f():
                _, h = F.cspn2d_forward_nl(aff, off, x, s, N_ITER, return_history=True)
                backward[k](aff, off, x, s, go, N_ITER, history=h)
            return f

        def sweeps(k, n):
            return lambda: backward[k](aff, off, x, s, go, n, 3, None, False, False, True)
        tb = blocks_of({k: bwd(k) for k in backward}, a.reps, a.blocks)
        tt = blocks_of({k: train(k) for k in backward}, a.reps, a.blocks)
        tx = blocks_of({"%s_%d" % (k, n): sweeps(k, n) for k in backward for n in (1, N_ITER)}, a.reps, a.blocks)
        for k in backward:
            row[k] = dict(bwd=stats(tb[k]), train=stats(tt[k]), bwd_mib=peak_mib(lambda: backward[k](aff, off, x, s, go, N_ITER, history=hist)), train_mib=peak_mib(train(k)),
                          grad_x_only_1=stats(tx[k + "_1"]), grad_x_only_n=stats(tx["%s_%d" % (k, N_ITER)]))
            t1, tn = row[k]["grad_x_only_1"]["ms"], row[k]["grad_x_only_n"]["ms"]
            row[k]["sweep_ms"] = round((tn - t1) / (N_ITER - 1), 3)
        d = row["deterministic"]
        d["index_build_ms"] = round(d["grad_x_only_1"]["ms"] - d["sweep_ms"], 3)
        again = backward["deterministic"](aff, off, x, s, go, N_ITER, history=hist)
        row["deterministic_twice_bitwise"] = all(torch.equal(p, q) for p, q in zip(grads["deterministic"], again))
        again = backward["scatter"](aff, off, x, s, go, N_ITER, history=hist)
        row["scatter_twice_bitwise"] = all(torch.equal(p, q) for p, q in zip(grads["scatter"], again))
        row.update({"rel_diff_" + n: rel(p, q) for n, p, q in zip(("daff", "doffset", "dx"), grads["deterministic"], grads["scatter"])})
        row["det_over_scatter_bwd"] = round(d["bwd"]["ms"] / row["scatter"]["bwd"]["ms"], 2)
        row["det_over_scatter_train"] = round(d["train"]["ms"] / row["scatter"]["train"]["ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del hist, grads, again
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    L = ["# The run-to-run bitwise backward of non-local propagation: `cspn2d_backward_nl_det` beside `cspn2d_backward_nl`", "",
         "Written by `tools/bench_nl_det.py` (reps %d, blocks %d) on %s, torch %s.  Shape KITTI x 8: B %d, C %d, %d x %d, n_iter %d, K 3; affinities randn * 0.2, "
         "~500 measured points per image (the setup of `tools/bench_nl.py`).  Times in ms: median (min - max) over the blocks of one run, the two variants taking "
         "turns.  No ratio is a pass condition; the scatter stays the default whichever way the figures fall."
         % (a.reps, a.blocks, torch.cuda.get_device_name(0), torch.__version__, B, C, H, W, N_ITER), "",
         "## Times", "",
         "| offsets | scatter backward | deterministic backward | det / scatter | scatter training step | deterministic training step | det / scatter |",
         "|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %s (std %.2f) | %s | %s | %.2f | %s | %s | %.2f |" % (
            r["offsets"], r["offset_std"], fmt(r["scatter"]["bwd"]), fmt(r["deterministic"]["bwd"]), r["det_over_scatter_bwd"], fmt(r["scatter"]["train"]),
            fmt(r["deterministic"]["train"]), r["det_over_scatter_train"]))
    L += ["", "The backward is all three gradients on a kept history; the training step is the forward that keeps its history, then that backward.", "",
          "## The index build apart from the sweeps", "",
          "T(n): the `grad_x`-only backward at n steps (the deterministic one: the index build and n gathered sweeps; the scatter: n memsets, n scattered "
          "sweeps and the pinning pass; neither runs the gate gradient).  A sweep is (T(%d) - T(1)) / %d; the index build is T(1) minus one sweep."
          % (N_ITER, N_ITER - 1), "",
          "| offsets | variant | T(1) | T(%d) | one sweep | index build |" % N_ITER, "|---|---|---|---|---|---|"]
    for r in rows:
        for k in ("scatter", "deterministic"):
            L.append("| %s | %s | %s | %s | %.3f | %s |" % (r["offsets"], k, fmt(r[k]["grad_x_only_1"]), fmt(r[k]["grad_x_only_n"]), r[k]["sweep_ms"],
                                                        "%.3f" % r[k]["index_build_ms"] if "index_build_ms" in r[k] else "-"))
    L += ["", "## Peak memory", "",
          "Peak bytes allocated by one call above what is allocated before it (MiB).  The workspace column is the size query's: the levels, and for the "
          "deterministic backward the index behind them (about 270 bytes a pixel: 8-byte entries for up to 32 taps a pixel, the starts, the cursors, the "
          "plane c, the worklist).", "",
          "| offsets | variant | backward alone | training step | workspace (query) |", "|---|---|---|---|---|"]
    for r in rows:
        for k in ("scatter", "deterministic"):
            L.append("| %s | %s | %.1f | %.1f | %.1f |" % (r["offsets"], k, r[k]["bwd_mib"], r[k]["train_mib"], r["workspace_mib"][k]))
    L += ["", "## Results at the timed size", "",
          "Two calls of the same backward compared bit for bit in all three gradients, and max |deterministic - scatter| / max |scatter| (both float32; the "
          "float64 comparisons are in `tests/test_nl_det.py`):", "",
          "| offsets | deterministic twice: same bits | scatter twice: same bits | grad_aff | grad_offset | grad_x |", "|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %s | %s | %s | %.2e | %.2e | %.2e |" % (r["offsets"], "yes" if r["deterministic_twice_bitwise"] else "NO", "yes" if r["scatter_twice_bitwise"] else "no",
                                                        r["rel_diff_daff"], r["rel_diff_doffset"], r["rel_diff_dx"]))
    L += ["", "## What the compiler made (not measured by this tool: read from the build)", "", BUILD_REPORT, ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("\n".join(L))


if __name__ == "__main__":
    main()
