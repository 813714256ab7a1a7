"""Line-scan propagation (cspn_amd.LineScan_Propagate: cspn2d_forward_scan / cspn2d_backward_scan) against the route it replaces, in the same
process on the same GPU:
    loop    the float32 torch statement under autograd: the clip rule, then per direction a Python loop over the lines (a handful of small torch
            kernels a step, one kept slice a step), then the maximum over the directions
    scan    the module with norm='clip', merge='max': torch's clip and max around one engine call forward and one backward
KITTI x 8 (B 8, 304 x 1216), four directions, (C, Cg) = (1, 1), (32, 32), (32, 1), without and with lam, float32.  The forward and one training step
(forward + backward to x, gates and lam) are timed.  The engine's forward is also timed on the horizontal pair (directions 0, 1: 1216 steps on
lines of 304 pixels) and the vertical pair (2, 3: 304 steps on lines of 1216 pixels) alone, with the time per step and the achieved bytes / s
against 8 TB/s; the bytes are the algorithmic ones, 4 (2 C + 3 Cg (+ C with lam)) per pixel and direction.
A time of `scan` is the median over the rounds of the per-round median of 5 prewarmed event-timed blocks of --reps calls, "spread" is (max - min) /
median over the rounds; a time of `loop` (seconds a call) is the median of three calls after one warm-up, its spread over those three.  Peak memory
is max_memory_allocated over one call less what was allocated before it; torch's clip and its backward work on the whole gate tensor in both
routes, so the peak of a training step is also taken on gates normalised beforehand, without a merge (the recurrence alone).  The maximum over the
directions is discontinuous where two directions tie within rounding, so the two routes' gradients are compared under merge='sum'.
    python tools/bench_scan.py [--reps 3] [--rounds 3] [--shape B H W] [--resources remarks.txt] [--out profiles/scan.md]
--resources: the compiler's -Rpass-analysis=kernel-resource-usage remarks of cspn2d_scan.hip, for the profile's resource table."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cspn_amd  # noqa: E402
from cspn_amd import functional as F  # noqa: E402
from cspn_amd import spn  # noqa: E402
from tools.bench_kxk import PEAK, timed  # noqa: E402
from tools.bench_kxk_dyn import med, peak_bytes  # noqa: E402

DIRS = (0, 1, 2, 3)
CONFIGS = ((1, 1), (32, 32), (32, 1))


def _canon(t, code):
    if code >= 2:
        t = t.transpose(-1, -2)
    return t.flip(-1) if code in (1, 3) else t


def _uncanon(t, code):
    if code in (1, 3):
        t = t.flip(-1)
    return t.transpose(-1, -2) if code >= 2 else t


def torch_loop(x, gates, lam=None, dirs=DIRS, norm="clip", merge="max"):
    """the contract with norm and merge as the module's, in float32 torch ops; the gates of a group broadcast over its channels"""
    B, C, H, W = x.shape
    D = len(dirs)
    Cg = gates.shape[1] // (3 * D)
    g = gates.reshape(B, D * Cg, 3, H, W)
    if norm == "clip":
        g = g / g.abs().sum(2, keepdim=True).clamp(min=1)
    g = g.reshape(B, D, Cg, 1, 3, H, W)
    outs = []
    for d, code in enumerate(dirs):
        gd = _canon(g[:, d], code)                                  # [B, Cg, 1, 3, L, T]
        xs = _canon(x.reshape(B, Cg, C // Cg, H, W), code)
        lm = None if lam is None else _canon(lam[:, d * C:(d + 1) * C].reshape(B, Cg, C // Cg, H, W), code)
        L, T = xs.shape[-2:]
        keep = torch.ones(3, L, device=x.device)
        keep[0, 0] = 0
        keep[2, L - 1] = 0
        h, lines = None, []
        for t in range(T):
            if t == 0:
                hn = xs[..., 0] if lm is None else lm[..., 0] * xs[..., 0]
            else:
                g0, g1, g2 = gd[:, :, :, 0, :, t] * keep[0], gd[:, :, :, 1, :, t], gd[:, :, :, 2, :, t] * keep[2]
                b = lm[..., t] if lm is not None else 1 - (g0 + g1 + g2)
                hm = torch.nn.functional.pad(h[..., :-1], (1, 0))
                hp = torch.nn.functional.pad(h[..., 1:], (0, 1))
                hn = b * xs[..., t] + g0 * hm + g1 * h + g2 * hp
            lines.append(hn)
            h = hn
        outs.append(_uncanon(torch.stack(lines, -1), code).reshape(B, 1, C, H, W))
    out = torch.cat(outs, 1)
    return out.max(1).values if merge == "max" else (out.sum(1) if merge == "sum" else out.reshape(B, D * C, H, W))


def timed_once(fn):
    """one warm-up, three event-timed calls -> (median ms, (max - min) / median): a call of the loop takes seconds"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[1], (ts[2] - ts[0]) / ts[1]


def resource_table(path):
    """the remarks file -> markdown rows: kernel, VGPRs, AGPRs, scratch, waves per SIMD, LDS bytes"""
    text = open(path).read()
    rows = []
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", text, re.S):
        k = re.search(r"(scan_[a-z]+_kernel)", m.group(1))
        if not k:
            continue
        row = "| `%s` | %s | %s | %s | %s | %s |" % ((k.group(1),) + m.groups()[1:])
        if row not in rows:
            rows.append(row)
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=(8, 304, 1216), metavar=("B", "H", "W"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    B, H, W = a.shape
    m = cspn_amd.LineScan_Propagate(DIRS, None, "clip", "max")
    rows = []
    for C, Cg in CONFIGS:
        for with_lam in (False, True):
            gen = torch.Generator(device="cuda").manual_seed(100 * C + Cg + int(with_lam))
            x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
            g = torch.randn(B, 4 * Cg * 3, H, W, device="cuda", generator=gen)
            lam = torch.rand(B, 4 * C, H, W, device="cuda", generator=gen) + 0.1 if with_lam else None
            go = torch.randn(B, C, H, W, device="cuda", generator=gen)
            leaves = [t.clone().requires_grad_(True) for t in (x, g) + ((lam,) if with_lam else ())]

            def step(route):
                for t in leaves:
                    t.grad = None
                out = route(*leaves)
                out.backward(go)
                return out

            def scan_fwd():
                with torch.no_grad():
                    return m(x, g, lam)

            def loop_fwd():
                with torch.no_grad():
                    return torch_loop(x, g, lam)

            gn = m.normalize(g).contiguous()
            pair = {}
            for label, dirs in (("horizontal", (0, 1)), ("vertical", (2, 3))):
                sel = [t for d in dirs for t in range(d * Cg * 3, (d + 1) * Cg * 3)]
                gp = gn[:, sel].contiguous()
                lp = None if lam is None else torch.cat([lam[:, d * C:(d + 1) * C] for d in dirs], 1).contiguous()
                pair[label] = (lambda gp=gp, lp=lp, dirs=dirs: F.cspn2d_forward_scan(x, gp, dirs, lp))

            fast = {"scan_fwd": scan_fwd, "scan_step": lambda: step(m), "horizontal_fwd": pair["horizontal"], "vertical_fwd": pair["vertical"]}
            slow = {"loop_fwd": loop_fwd, "loop_step": lambda: step(torch_loop)}
            ts = {k: [] for k in fast}
            for _ in range(a.rounds):
                for k, fn in fast.items():
                    ts[k].append(timed(fn, a.reps))
            t = {k: med(v) for k, v in ts.items()}
            spread = {k: (max(v) - min(v)) / t[k] for k, v in ts.items()}
            for k, fn in slow.items():
                t[k], spread[k] = timed_once(fn)
            mem = {k: peak_bytes(fn) for k, fn in list(fast.items())[:2] + list(slow.items())}
            bare = [t.clone().requires_grad_(True) for t in (x, gn) + ((lam,) if with_lam else ())]
            gob = torch.randn(B, 4 * C, H, W, device="cuda", generator=gen)

            def bare_step(route):
                for t in bare:
                    t.grad = None
                route(*bare).backward(gob)

            mem["scan_bare_step"] = peak_bytes(lambda: bare_step(lambda *a_: spn.linescan_propagate(a_[0], a_[1], DIRS, a_[2] if with_lam else None)))
            mem["loop_bare_step"] = peak_bytes(lambda: bare_step(lambda *a_: torch_loop(*a_, norm=None, merge=None)))
            del bare, gob
            ref, got = loop_fwd(), scan_fwd()
            err = float((ref - got).abs().max() / ref.abs().max())
            msum = cspn_amd.LineScan_Propagate(DIRS, None, "clip", "sum")
            step(lambda *a_: torch_loop(*a_, merge="sum"))
            ref_g = [t_.grad.clone() for t_ in leaves]
            step(msum)
            gerr = [float((r - t_.grad).abs().max() / r.abs().max()) for r, t_ in zip(ref_g, leaves)]
            pair_bytes = 2 * B * H * W * 4 * (2 * C + 3 * Cg + (C if with_lam else 0))
            row = dict(B=B, C=C, Cg=Cg, H=H, W=W, lam=with_lam, rounds=a.rounds, reps=a.reps, **{k + "_ms": round(v, 3) for k, v in t.items()},
                       **{k + "_spread": round(v, 4) for k, v in spread.items()}, **{k + "_peak_mb": round(v / 2 ** 20, 1) for k, v in mem.items()},
                       fwd_ratio=round(t["loop_fwd"] / t["scan_fwd"], 2), step_ratio=round(t["loop_step"] / t["scan_step"], 2),
                       horizontal_us_per_step=round(1e3 * t["horizontal_fwd"] / W, 3), vertical_us_per_step=round(1e3 * t["vertical_fwd"] / H, 3),
                       horizontal_roofline=round(pair_bytes / (t["horizontal_fwd"] * 1e-3) / PEAK, 4),
                       vertical_roofline=round(pair_bytes / (t["vertical_fwd"] * 1e-3) / PEAK, 4),
                       horizontal_to_vertical=round(t["horizontal_fwd"] / t["vertical_fwd"], 3), fwd_max_rel_diff=err, grad_max_rel_diff=gerr)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, g, lam, go, leaves, ref, got, ref_g, gn, pair, fast, slow
            torch.cuda.empty_cache()
    lines = ["# Line-scan propagation (`cspn2d_*_scan_*`, DESIGN.md §3.4l)", "", "Written by `tools/bench_scan.py`; the only source of figures for §3.4l.", ""]
    if a.resources:
        lines += ["## Resources of every kernel (gfx950, `-Rpass-analysis=kernel-resource-usage`)", "",
                  "Each kernel has one instance: the orientation of a workgroup's lines is a branch on its direction.  None uses scratch.", "",
                  "| kernel | VGPRs | AGPRs | scratch bytes / lane | waves / SIMD | LDS bytes / workgroup |", "|---|---|---|---|---|---|"]
        lines += resource_table(a.resources) + [""]
    lines += ["## Measured on one MI355X: %s, B %d, %d x %d, four directions, float32" % (torch.cuda.get_device_name(0), B, H, W), "",
              "`loop`: the float32 torch statement under autograd (clip, a Python loop over the lines of every direction, max); `scan`: "
              "`LineScan_Propagate(norm='clip', merge='max')`.  `scan`: median over %d rounds of the per-round median of 5 blocks of %d calls, spread = (max - min) "
              "/ median over the rounds; `loop`: median of three calls after one warm-up, spread over those three.  Peak = `max_memory_allocated` over one "
              "call less what was allocated before it; torch's clip and its backward work on the whole gate tensor in both routes and set the peak of "
              "the training step, so the last peak column is the recurrence alone (gates normalised beforehand, no merge).  The gradients are compared "
              "under `merge='sum'` (the maximum is discontinuous where two directions tie within rounding).  A ratio above 1 means `scan` is faster."
              % (a.rounds, a.reps), "",
              "| C | Cg | lam | forward loop ms (spread) | forward scan ms (spread) | ratio | training step loop ms (spread) | training step scan ms (spread) | ratio | "
              "peak forward loop / scan MiB | peak training step loop / scan MiB | peak training step of the recurrence alone loop / scan MiB | "
              "max rel. difference out / dL/dx, dL/dgates[, dL/dlam] |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %d | %s | %.2f (%.1f %%) | %.3f (%.1f %%) | %.1f | %.2f (%.1f %%) | %.3f (%.1f %%) | %.1f | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.2g / %s |" % (
            r["C"], r["Cg"], "yes" if r["lam"] else "no", r["loop_fwd_ms"], 100 * r["loop_fwd_spread"], r["scan_fwd_ms"], 100 * r["scan_fwd_spread"],
            r["fwd_ratio"], r["loop_step_ms"], 100 * r["loop_step_spread"], r["scan_step_ms"], 100 * r["scan_step_spread"], r["step_ratio"],
            r["loop_fwd_peak_mb"], r["scan_fwd_peak_mb"], r["loop_step_peak_mb"], r["scan_step_peak_mb"], r["loop_bare_step_peak_mb"], r["scan_bare_step_peak_mb"], r["fwd_max_rel_diff"],
            ", ".join("%.2g" % e for e in r["grad_max_rel_diff"])))
    lines += ["", "## The engine's forward on the two pairs of directions alone", "",
              "Horizontal: directions 0 and 1, %d steps on lines of %d pixels; vertical: directions 2 and 3, %d steps on lines of %d pixels.  Both pairs "
              "move the same bytes; the share is of 8 TB/s." % (W, H, H, W), "",
              "| C | Cg | lam | horizontal ms (spread) | us / step | share of the roofline | vertical ms (spread) | us / step | share of the roofline | horizontal / vertical |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %d | %s | %.3f (%.1f %%) | %.3f | %.4f | %.3f (%.1f %%) | %.3f | %.4f | %.2f |" % (
            r["C"], r["Cg"], "yes" if r["lam"] else "no", r["horizontal_fwd_ms"], 100 * r["horizontal_fwd_spread"], r["horizontal_us_per_step"],
            r["horizontal_roofline"], r["vertical_fwd_ms"], 100 * r["vertical_fwd_spread"], r["vertical_us_per_step"], r["vertical_roofline"],
            r["horizontal_to_vertical"]))
    lines += ["", "Raw rows:", "", "```"] + [json.dumps(r) for r in rows] + ["```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
