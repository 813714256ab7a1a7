"""The 3D depth-completion contract on fp16 / bf16 guidance at config 5's volume (4 x 26 x 32 x 160 x 608), n_iter 12, '8sum_abs', without a
mask and with 5 % of the voxels pinned, in one process on one GPU.  Two routes through cspn_amd.Affinity_Propagate3d:
    cast    guidance.float() in front of the module: the float32 engine on a float32 copy, the gradient cast back by autograd
            (what the module itself did with a 16-bit guidance before cspn3d_*_norm_g16 existed)
    native  the 16-bit guidance handed to the module as it is (cspn3d_forward_norm_g16 / cspn3d_backward_norm_g16)
Per cell (dtype x mask): the forward alone (no_grad), one training step (forward + backward, both gradients), and the peak of
torch.cuda.max_memory_allocated over one training step above what the inputs hold.  A time is the median of event-timed blocks after a
warm-up; min and max are printed next to it.  --root imports cspn_amd from another checkout with its library built: the same script then
measures the 'cast' route on the code of another commit, in the same session (run the two alternately; the spread between two runs of the
same code is the margin of the comparison).
    python tools/bench_3d_norm_g16.py --route native|cast [--root DIR] [--json out.json] [--shape B D H W] [--n-iter 12]"""
import argparse
import json
import os
import statistics
import sys


def timed(torch, fn, warm, blocks, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("native", "cast"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default=None)
    ap.add_argument("--shape", type=int, nargs=4, default=(4, 32, 160, 608), metavar=("B", "D", "H", "W"))
    ap.add_argument("--n-iter", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=8)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import cspn_amd
    assert os.path.abspath(cspn_amd.__file__).startswith(os.path.abspath(a.root)), "cspn_amd was not imported from --root"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    (B, D, H, W), N, norm = a.shape, a.n_iter, "8sum_abs"
    gen = torch.Generator(device="cuda").manual_seed(0)
    g = torch.rand(B, 26, D, H, W, generator=gen, device="cuda") - 0.3
    feat = torch.rand(B, 1, D, H, W, generator=gen, device="cuda")
    go = torch.randn(B, 1, D, H, W, generator=gen, device="cuda")
    sparse5 = (torch.rand(B, 1, D, H, W, generator=gen, device="cuda") < 0.05).float() * (feat + 0.1)
    module = cspn_amd.Affinity_Propagate3d(N, 3, norm)
    res = {"route": a.route, "root": os.path.abspath(a.root), "shape": [B, D, H, W], "n_iter": N, "norm_type": norm, "cells": {}}
    for dtype in (torch.float16, torch.bfloat16):
        g16 = g.to(dtype)
        for name, sp in (("no_mask", None), ("mask_5pct", sparse5)):

            def forward():
                with torch.no_grad():
                    return module(g16.float() if a.route == "cast" else g16, feat, sp)

            def step():
                g1, f1 = g16.detach().requires_grad_(True), feat.detach().requires_grad_(True)
                out = module(g1.float() if a.route == "cast" else g1, f1, sp)
                out.backward(go)
                return out, g1.grad, f1.grad

            out, gg, gf = step()
            cspn_amd.cspn3d_check_status()
            assert out.dtype == torch.float32 and gg.dtype == dtype and gf.dtype == torch.float32
            # (a checksum: the two routes compute the same numbers, so these agree between the runs that are compared)
            row = {"checksum": {"out": float(out.double().sum()), "grad_guidance": float(gg.double().nan_to_num().abs().sum()),
                                "grad_feat": float(gf.double().sum())}}
            del out, gg, gf
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            kept = step()
            torch.cuda.synchronize()
            row["step_peak_bytes_above_inputs"] = torch.cuda.max_memory_allocated() - base
            del kept
            row["forward"] = timed(torch, forward, 3, a.blocks, a.reps)
            row["forward_backward"] = timed(torch, step, 3, a.blocks, a.reps)
            cspn_amd.cspn3d_check_status()
            res["cells"]["%s/%s" % (str(dtype).replace("torch.", ""), name)] = row
            print(a.route, dtype, name, json.dumps(row), flush=True)
        del g16
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
