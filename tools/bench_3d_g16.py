"""The 3D engine on fp16 / bf16 gates (cspn3d_*_g16) at config 5 (4 x 26 x 32 x 160 x 608) against the two float32 routes, in one process
on one GPU.  Per row and 16-bit type:
    cast   today's route for a 16-bit head: a differentiable gate.float() in front of the float32 engine (and, in training, autograd's
           rounding of the float32 gate gradient back to the gate's dtype)
    f32    the float32 engine on gates widened outside the timed region (for information)
    g16    the 16-bit gates handed to the engine as they are
Rows: the NONE op's forward (n = 12), the demo module's forward (n = 12), forward + backward through affinity_propagate at n = 12 and n = 1.
The variants alternate within a round and the rounds repeat; a time is the median over the rounds of the per-round median of 5 prewarmed
event-timed blocks, "spread" is (max - min) / median of a variant over the rounds -- cast's is the yardstick for "not slower".  Also: the
peak memory of one training step of CSPN(3, 1, 3, 12) on both routes, and whether the outputs are bitwise equal at the timed size.
A library built before the 16-bit entry points (CSPN_AMD_LIB=<path to its libcspn_amd.so>) measures cast and f32 only: the baseline on
the parent commit's kernels.
    python tools/bench_3d_g16.py [--reps 5] [--rounds 5] [--json out.jsonl] [--shape B D H W]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cspn_amd  # noqa: E402
from cspn_amd import functional as F  # noqa: E402
from tools.bench_kxk import timed  # noqa: E402


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--shape", type=int, nargs=4, default=(4, 32, 160, 608), metavar=("B", "D", "H", "W"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    B, D, H, W = a.shape
    have16 = hasattr(cspn_amd.load(), "cspn3d_forward_g16_algo")
    rows = []
    for dtype in (torch.float16, torch.bfloat16):
        gen = torch.Generator(device="cuda").manual_seed(5)
        g = torch.randn(B, 26, D, H, W, device="cuda", generator=gen)
        g16 = (g / g.abs().sum(1, keepdim=True)).to(dtype)
        del g
        g32 = g16.float()
        x = torch.rand(B, 1, D, H, W, device="cuda", generator=gen)
        go = torch.randn(B, 1, D, H, W, device="cuda", generator=gen)
        g16r, g32r, xr = g16.clone().requires_grad_(True), g32.clone().requires_grad_(True), x.clone().requires_grad_(True)

        def train(gate, n, cast):
            g16r.grad = g32r.grad = xr.grad = None
            cspn_amd.affinity_propagate(xr, gate.float() if cast else gate, 3, n).backward(go)

        ops = {
            "none_fwd_n12": {"cast": lambda: F.cspn3d_forward(g16.float(), x, None, 12, "none"),
                             "f32": lambda: F.cspn3d_forward(g32, x, None, 12, "none"),
                             "g16": lambda: F.cspn3d_forward(g16, x, None, 12, "none")},
            "demo_fwd_n12": {"cast": lambda: F.cspn3d_forward_absnorm(g16.float(), x, 12),
                             "f32": lambda: F.cspn3d_forward_absnorm(g32, x, 12),
                             "g16": lambda: F.cspn3d_forward_absnorm(g16, x, 12)},
            "none_fwd_bwd_n12": {"cast": lambda: train(g16r, 12, True), "f32": lambda: train(g32r, 12, False), "g16": lambda: train(g16r, 12, False)},
            "none_fwd_bwd_n1": {"cast": lambda: train(g16r, 1, True), "f32": lambda: train(g32r, 1, False), "g16": lambda: train(g16r, 1, False)},
        }
        for name, variants in ops.items():
            if not have16:
                variants = {k: v for k, v in variants.items() if k != "g16"}
            with torch.set_grad_enabled("bwd" in name):
                ts = {k: [] for k in variants}
                for _ in range(a.rounds):
                    for k, fn in variants.items():
                        ts[k].append(timed(fn, a.reps))
            F.cspn3d_check_status()
            row = dict(op=name, dtype=str(dtype).replace("torch.", ""), B=B, D=D, H=H, W=W, rounds=a.rounds, lib_has_g16=have16)
            for k, v in ts.items():
                row[k + "_ms"] = round(med(v), 4)
                row[k + "_spread"] = round((max(v) - min(v)) / med(v), 4)
            if have16:
                row["g16_vs_cast"] = round(med(ts["cast"]) / med(ts["g16"]), 3)
                row["g16_vs_f32"] = round(med(ts["f32"]) / med(ts["g16"]), 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
        if have16:
            with torch.no_grad():
                same = bool(torch.equal(F.cspn3d_forward(g16, x, None, 12, "none"), F.cspn3d_forward(g32, x, None, 12, "none")))
                same_demo = bool(torch.equal(F.cspn3d_forward_absnorm(g16, x, 12), F.cspn3d_forward_absnorm(g32, x, 12)))
            row = dict(op="bitwise", dtype=str(dtype).replace("torch.", ""), none_fwd_equal=same, demo_fwd_equal=same_demo)
            rows.append(row)
            print(json.dumps(row), flush=True)
        # peak memory of one training step of the demo module, both routes (the guide is the head's output: allocated before the step)
        del g32, g32r
        torch.cuda.empty_cache()
        m = cspn_amd.CSPN(3, 1, 3, 12)
        peaks = {}
        for route in ("cast", "g16") if have16 else ("cast",):
            for _ in range(2):   # (the second step is the one reported: no one-time allocations in it)
                g16r.grad = xr.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                m(g16r.float() if route == "cast" else g16r, xr).backward(go)
                torch.cuda.synchronize()
                peaks[route] = torch.cuda.max_memory_allocated() - base
        F.cspn3d_check_status()
        row = dict(op="CSPN(3,1,3,12) training step, peak memory over the resident inputs", dtype=str(dtype).replace("torch.", ""),
                   **{k + "_peak_MB": round(v / 1e6, 1) for k, v in peaks.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del g16, g16r, x, xr, go
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
