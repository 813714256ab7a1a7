"""C channels on shared 3D guidance at config 5's volume: the loop of C Affinity_Propagate3d calls (whatever cspn_amd is first on the path)
against the one-call route.  One JSON line per measurement, appended to --out."""
import argparse
import json
import statistics
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--impl", choices=("loop", "multi"), required=True)
ap.add_argument("--tag", default="")
ap.add_argument("--out", required=True)
ap.add_argument("--shape", default="4,32,160,608")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

import cspn_amd

if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured")
B, D, H, W = (int(x) for x in args.shape.split(","))
N, NORM = 12, "8sum_abs"


def inputs(C, mask):
    torch.manual_seed(1234 + C)
    g = torch.randn(B, 26, D, H, W, device="cuda")
    f = torch.rand(B, C, D, H, W, device="cuda")
    go = torch.randn(B, C, D, H, W, device="cuda")
    s = None
    if mask:
        s = (torch.rand(B, 1, D, H, W, device="cuda") < 0.05).float() * (f[:, :1] + 0.1)
    return g, f, s, go


def loop(m, g, f, s):
    return torch.cat([m(g, f[:, c:c + 1].contiguous(), s) for c in range(f.shape[1])], 1)


def multi(m, g, f, s):
    return m(g, f, s)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def emit(rec):
    rec.update(impl=args.impl, tag=args.tag, shape=[B, D, H, W], n_iter=N, norm=NORM)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


run = loop if args.impl == "loop" else multi
for C in (2, 4):
    for mask in (False, True):
        g, f, s, go = inputs(C, mask)
        for algo in (("auto",) if args.impl == "loop" else ("stepwise", "auto")):
            m = cspn_amd.Affinity_Propagate3d(N, 3, NORM)
            m.algo = algo
            with torch.no_grad():
                med, lo, hi = timed(lambda: run(m, g, f, s), args.reps)
            emit(dict(what="forward", C=C, mask=mask, algo=algo, ms_median=med, ms_min=lo, ms_max=hi))
            gr, fr = g.clone().requires_grad_(True), f.clone().requires_grad_(True)

            def step():
                gr.grad = None
                fr.grad = None
                run(m, gr, fr, s).backward(go)
            med, lo, hi = timed(step, max(args.reps // 2, 3))
            gr.grad = None
            fr.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            emit(dict(what="train_step", C=C, mask=mask, algo=algo, ms_median=med, ms_min=lo, ms_max=hi, peak_bytes=peak, resident_before_bytes=base,
                      step_bytes=peak - base))
            cspn_amd.cspn3d_check_status()
            if args.impl == "multi" and C == 2:
                # the same numbers as the loop of single-channel calls of this library, on the inputs that were timed
                ref = loop(m, gr, fr, s)
                gr.grad = None
                fr.grad = None
                out = multi(m, gr, fr, s)
                d_out = float((out - ref).abs().max() / ref.abs().max())
                out.backward(go)
                gg, gf = gr.grad.clone(), fr.grad.clone()
                gr.grad = None
                fr.grad = None
                ref.backward(go)
                d_gg = float((gg - gr.grad).abs().max() / gr.grad.abs().max())
                d_gf = float((gf - fr.grad).abs().max() / fr.grad.abs().max())
                emit(dict(what="multi_vs_loop_max_norm", C=C, mask=mask, algo=algo, out=d_out, grad_guidance=d_gg, grad_feat=d_gf))
            del gr, fr
        del g, f, s, go
        torch.cuda.empty_cache()
