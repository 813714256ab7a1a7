"""fp16 / bf16 affinities and offsets in non-local propagation (cspn2d_*_nl*_g16) beside THE ROUTE THEY REPLACE, measured on the parent commit:
.float() of the 16-bit tensors, the float32 functions, .to(dtype) of the gradients that belong to 16-bit tensors.  Writes profiles/nl_g16.md, the
only source of the figures README.md and DESIGN.md §3.4j quote for the 16-bit route.
Shape and inputs are tools/bench_nl.py's: KITTI x 8 (B 8, 1 x 304 x 1216), n_iter 18, C 1, affinities randn * 0.2, ~500 measured points per image,
offsets `random` (randn * 1.5) and `smooth` (a 15 x 15 box low-pass of the same draw at the same standard deviation), the same reps and blocks.
Per dtype (fp16, bf16) and pair ((float32 aff, T offset): what NonLocal_Propagate hands the engine; (T, T)): the forward, the training step (the
forward that keeps its history, then the backward for all three gradients) with the scatter and with the deterministic backward, and the peak
memory of those steps.  The float32 engine is timed in both runs, to show the existing path did not move.
Two runs, one process each, one after the other in the same session:
    python tools/bench_nl_g16.py --baseline --root <checkout of the parent commit, built> --json base.jsonl
        imports nothing this commit adds: the parent's route and the parent's float32 engine
    python tools/bench_nl_g16.py --baseline-json base.jsonl [--md profiles/nl_g16.md] [--json new.jsonl]
        the 16-bit route and this commit's float32 engine; writes the profile
The condition, stated either way in the profile: each 16-bit median no slower than the parent route's median by more than the parent's own block
spread ((max - min) / median, as measured), and the training steps' peak memory lower than the parent route's.  No ratio is fixed in advance."""
import argparse
import json
import os
import sys

import torch

KK, N_ITER, C = 8, 18, 1
B, H, W = 8, 304, 1216
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
PAIRS = ("0T", "TT")
WHATS = ("fwd", "train", "train_det")

# what the compiler reports for cspn_amd/csrc/cspn2d_nl.hip and cspn2d_nl_det.hip (hipcc -O3 --offload-arch=gfx950, the per-kernel summary of the
# device assembly): not measured by this tool, recorded here so that the profile has one source.  T stands for fp16 and bf16, whose figures agree
# except where both are given
BUILD_REPORT = """\
| kernel | instance (aff, offset) | VGPRs | AGPRs | scratch | occupancy (waves / SIMD) | `profiles/nl.md` (float32) |
|---|---|---|---|---|---|---|
| `nl_forward_step<3, VEC>` | (float, float) | 242 | 0 | 0 | 2 | 242 / 0 / 0 / 2 |
| | (float, T) | 236 | 0 | 0 | 2 | |
| | (T, T) | 236 | 0 | 0 | 2 | |
| `nl_forward_step<3, scalar>` | (float, float) | 256 | 86 | 0 | 1 | 256 / 86 / 0 / 1 |
| | (float, T), (T, T) | 256 | 86 | 0 | 1 | |
| `nl_adjoint_step<3>` (LDS window 8,512 bytes in every instance) | (float, float) | 52 | 0 | 0 | 8 | 52 / 0 / 0 / 8 |
| | (float, T), (T, T) | 52 | 0 | 0 | 8 | |
| `nl_gate_grad<3>` | (float, float) | 128 | 0 | 0 | 4 | 128 / 0 / 0 / 4 |
| | (float, T), (T, T) | 128 | 0 | 0 | 4 | |
| `nl_sample_kernel<3>` | float | 49 | 0 | 0 | 8 | 49 / 0 / 0 / 8 |
| | fp16 / bf16 | 54 / 53 | 0 | 0 | 8 | |
| `nl_sample_backward_kernel<3>` | float, fp16, bf16 | 26 | 0 | 0 | 8 | (32 when `profiles/nl.md` was written; 26 at the parent commit) |
| `nl_index_taps<3, count / fill>` | every pair | 34 / 28 | 0 | 0 | 8 | |

No instance uses scratch, and the float32 instances keep the register counts of `profiles/nl.md`: 242, 256 + 86 AGPR, 52 and 128.  Compared
instruction by instruction with a build of the parent commit, the float32 instances of `nl_forward_step` (both), `nl_adjoint_step`, `nl_gate_grad`,
`nl_sample_kernel`, `nl_sample_backward_kernel`, `nl_index_taps` (both), `nl_pin` and every kernel of the index and the gathers are the parent's
code.  For `nl_adjoint_step` that took one change: with five instances in the unit the compiler merged the LDS add and the global add of
`scatter_add` into one flat atomic on a selected address (32 `flat_atomic_add_f32` in every instance, the float32 one included); the LDS add now
names workgroup scope, the two stay apart (33 `ds_add_f32`, 35 `global_atomic_add_f32` per instance) and the float32 instance is the parent's
1,658 instructions again.
The 16-bit vector forward needs 6 registers fewer than the float32 one (the 24 planes arrive in half the load registers) and stays at two waves
per SIMD: the affinities, fractions and corner indices it keeps over the channel loop are float32 / int32 after the widening, and they are what
fills the register file.  So the 16-bit forward streams 48 instead of 96 bytes of affinities and offsets per pixel and step at the occupancy of
the float32 kernel."""


# where the time condition fails: the cause as far as the build's report shows it (written into the profile only then)
WHY_SLOWER = """\
**No speed-up is claimed; the 16-bit route stands on its results and on the memory above.**  Where the rows say NO, the cause as far as the
build's report (below) shows it: the 16-bit vector forward is no leaner a kernel than the float32 one -- 236 against 242 VGPRs, the same two
waves per SIMD, the same number of load instructions (24 a thread and step, each half as wide) -- and it adds the widening: four unpack /
convert instructions per quad, 64 (pair `0T`) or 96 (pair `TT`) a thread and step, in front of the same `tap_of` arithmetic.  At 28 % of
the bandwidth roofline (`profiles/nl.md`) the step is bound by instruction issue and latency at that occupancy, not by the 48 bytes a pixel
and step it no longer reads, so the added instructions show (the forward's extra time grows with the number of 16-bit planes: 16 in `0T`,
24 in `TT`) and the saved bytes do not.  The parent route pays for its casts once per call (about 0.07 ms for the 24 planes), the 16-bit
route widens again on each of the 18 steps.  The training steps differ by what their forward differs by: the adjoint is bound by LDS adds
and the gate gradient reads each plane once.  Keeping the affinities packed across the channel loop (not tried here) would free 16 of the
128 registers the thread keeps over that loop (corner indices, fractions, affinities of 8 neighbours x 4 pixels); a third wave needs 168 or fewer in all."""


def blocks_of(fns, reps, blocks):
    """fns: name -> callable; the callables take turns block by block -> name -> sorted per-call times (ms)"""
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) / reps)
    return {k: sorted(v) for k, v in ts.items()}


def stats(v):
    med = v[len(v) // 2]
    return dict(ms=round(med, 3), min=round(v[0], 3), max=round(v[-1], 3), spread=round((v[-1] - v[0]) / med, 4))


def peak_mib(f):
    """peak bytes allocated by one call of f above what is allocated before it, in MiB"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def fmt(s):
    return "%.3f (%.3f - %.3f)" % (s["ms"], s["min"], s["max"])


def inputs():
    gen = torch.Generator(device="cuda").manual_seed(18)
    aff = torch.randn(B, KK, H, W, device="cuda", generator=gen) * 0.2
    draw = torch.randn(B, 2 * KK, H, W, device="cuda", generator=gen) * 1.5
    low = torch.nn.functional.avg_pool2d(draw, 15, 1, 7)
    fields = {"random": draw.contiguous(), "smooth": (low * (draw.std() / low.std())).contiguous()}
    x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
    s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 500 / (H * W)).float() * (x[:, :1] * 0.5 + 0.1)
    go = torch.randn(B, C, H, W, device="cuda", generator=gen)
    return aff, fields, x, s, go


def routes(F, baseline, a, o, x, s, go):
    """name -> callable for one (aff, offset) as the caller holds them.  baseline: the route a port takes without 16-bit entry points (names of the
    parent commit only); else the *_g16 functions on the tensors as they are.  float32 aff and offset: the float32 functions in both runs"""
    f32 = a.dtype == torch.float32 and o.dtype == torch.float32
    if baseline or f32:
        fwd, bwd = F.cspn2d_forward_nl, {False: F.cspn2d_backward_nl, True: F.cspn2d_backward_nl_det}

        def widened():   # .float() is a no-op on a float32 tensor
            return a.float(), o.float()

        def narrowed(ga, gd, gx):
            return ga.to(a.dtype), gd.to(o.dtype), gx
    else:
        fwd, bwd = F.cspn2d_forward_nl_g16, {False: F.cspn2d_backward_nl_g16, True: F.cspn2d_backward_nl_det_g16}

        def widened():
            return a, o

        def narrowed(ga, gd, gx):
            return ga, gd, gx

    def forward():
        aw, ow = widened()
        return fwd(aw, ow, x, s, N_ITER)

    def train(det):
        def step():
            aw, ow = widened()
            out, hist = fwd(aw, ow, x, s, N_ITER, return_history=True)
            return (out,) + narrowed(*bwd[det](aw, ow, x, s, go, N_ITER, history=hist))
        return step
    return {"fwd": forward, "train": train(False), "train_det": train(True)}


def measure(F, baseline, reps, blocks):
    aff, fields, x, s, go = inputs()
    rows = []
    for name, off in fields.items():
        cases = [("f32", "f32", aff, off)]
        for dn, dt in DTYPES.items():
            for pair in PAIRS:
                cases.append((dn, pair, aff.to(dt) if pair == "TT" else aff, off.to(dt)))
        for dn, pair, a, o in cases:
            fns = routes(F, baseline, a, o, x, s, go)
            row = dict(offsets=name, dtype=dn, pair=pair, baseline=bool(baseline))
            for what in WHATS:
                row[what] = stats(blocks_of({what: fns[what]}, reps, blocks)[what])
            for what in WHATS[1:]:
                row[what + "_mib"] = peak_mib(fns[what])
            row["fwd_mib"] = peak_mib(fns["fwd"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del fns
            torch.cuda.empty_cache()
    return rows


def key(r):
    return (r["offsets"], r["dtype"], r["pair"])


def write_profile(path, base, new, reps, blocks):
    base, new = {key(r): r for r in base}, {key(r): r for r in new}
    fails = []
    L = ["# Non-local propagation on fp16 / bf16 affinities and offsets: the `_g16` entry points beside the route they replace", "",
         "Written by `tools/bench_nl_g16.py` (reps %d, blocks %d) on %s, torch %s.  Shape KITTI x 8: B %d, C %d, %d x %d, n_iter %d, K 3; the inputs of "
         "`tools/bench_nl.py`.  Times in ms: median (min - max) over the blocks of one run." % (reps, blocks, torch.cuda.get_device_name(0), torch.__version__, B, C, H, W, N_ITER), "",
         "**Parent route**: measured on a build of the parent commit in the same session, with names that exist there: `.float()` of the 16-bit tensors, "
         "`cspn2d_forward_nl` / `cspn2d_backward_nl` / `cspn2d_backward_nl_det`, `.to(dtype)` of the gradients of the 16-bit tensors.  **16-bit route**: this "
         "commit's `_g16` functions on the tensors as they are.  Pair `0T`: float32 affinities (what `NonLocal_Propagate` hands the engine after normalising "
         "in float32) on 16-bit offsets; `TT`: both 16-bit.  The training step is the forward that keeps its history and the backward for all three gradients, "
         "with the scatter (`train`) or the deterministic backward (`train det`).", "",
         "## Times", "",
         "| offsets | dtype | pair | what | parent route | 16-bit route | 16-bit / parent | parent's block spread | within the condition |", "|---|---|---|---|---|---|---|---|---|"]
    for k in sorted(new):
        if k[1] == "f32":
            continue
        for what in WHATS:
            p, n = base[k][what], new[k][what]
            ok = n["ms"] <= p["ms"] * (1 + p["spread"])
            if not ok:
                fails.append("%s %s %s %s: %.3f ms against %.3f ms (spread %.2f %%)" % (k + (what, n["ms"], p["ms"], 100 * p["spread"])))
            L.append("| %s | %s | %s | %s | %s | %s | %.3f | %.2f %% | %s |" % (k + (what.replace("_", " "), fmt(p), fmt(n), n["ms"] / p["ms"], 100 * p["spread"], "yes" if ok else "NO")))
    L += ["", "## Peak memory of one call (MiB allocated above the inputs)", "",
          "| offsets | dtype | pair | forward: parent | forward: 16-bit | train: parent | train: 16-bit | train det: parent | train det: 16-bit |", "|---|---|---|---|---|---|---|---|---|"]
    mem_fails = []
    for k in sorted(new):
        if k[1] == "f32":
            continue
        p, n = base[k], new[k]
        for what in WHATS[1:]:
            if not n[what + "_mib"] < p[what + "_mib"]:
                mem_fails.append("%s %s %s %s: %.1f MiB against %.1f MiB" % (k + (what, n[what + "_mib"], p[what + "_mib"])))
        L.append("| %s | %s | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (k + (p["fwd_mib"], n["fwd_mib"], p["train_mib"], n["train_mib"], p["train_det_mib"], n["train_det_mib"])))
    L += ["", "## The condition", "",
          "Each 16-bit median no slower than the parent route's median by more than the parent's own block spread ((max - min) / median, as measured): %s."
          % ("holds in all %d rows" % (len([k for k in new if k[1] != "f32"]) * len(WHATS)) if not fails else "DOES NOT HOLD in %d rows -- %s" % (len(fails), "; ".join(fails))), "",
          "Peak memory of the training step lower than the parent route's: %s." % ("holds in every row" if not mem_fails else "DOES NOT HOLD -- " + "; ".join(mem_fails)), "",
          "No ratio was fixed in advance and none is claimed beyond the rows above.", ""] + ([WHY_SLOWER, ""] if fails else []) + [
          "## The float32 engine on both commits (the existing path)", "",
          "| offsets | what | parent commit | this commit | this / parent |", "|---|---|---|---|---|"]
    for k in sorted(new):
        if k[1] != "f32":
            continue
        for what in WHATS:
            p, n = base[k][what], new[k][what]
            L.append("| %s | %s | %s | %s | %.3f |" % (k[0], what.replace("_", " "), fmt(p), fmt(n), n["ms"] / p["ms"]))
    L += ["", "## What the compiler made (not measured by this tool: read from the cross-compiled build)", "", BUILD_REPORT, ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--baseline", action="store_true", help="the parent route and the float32 engine with names of the parent commit only")
    ap.add_argument("--root", default=here, help="the checkout whose cspn_amd is measured (a built checkout of the parent commit with --baseline)")
    ap.add_argument("--baseline-json", default=None, help="what the --baseline run wrote; needed to write the profile")
    ap.add_argument("--md", default=os.path.join(here, "profiles", "nl_g16.md"))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from cspn_amd import functional as F
    assert os.path.abspath(F.__file__).startswith(os.path.abspath(a.root)), (F.__file__, a.root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_nl_g16.py measures on the GPU; none found")
    rows = measure(F, a.baseline, a.reps, a.blocks)
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not a.baseline and a.baseline_json:
        with open(a.baseline_json) as f:
            base = [json.loads(line) for line in f if line.strip()]
        write_profile(a.md, base, rows, a.reps, a.blocks)


if __name__ == "__main__":
    main()
