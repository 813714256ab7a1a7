#!/usr/bin/env python
"""tools/bench_normalize_backward.py [--kernel-only] -- the backward of the normalisation (profiles/normalize_backward.md).

1. cspn2d_normalize_backward_f32 alone at KITTI x 64 (B 64, 304 x 1216), both norms: device events, warmed, median of 3 blocks of 20 launches;
   ms and TB/s on the algorithmic 96 B/pixel (raw guidance + dL/dgate_wb read, dL/dguidance written).
2. One training step (forward + loss + backward to the feature map and both head weights) of each route, B 8 and 64 (C 64, 152 x 608 -> 304 x 1216,
   24 iterations, training mode):
     raw:     guidance_heads(x, w6, w5) -> Affinity_Propagate(24, 3, '8sum')        (the normalisation's backward inside cspn2d_backward)
     prenorm: guidance_heads(x, w6, w5, norm_type='8sum') -> propagate_prenorm      (raw heads + cspn2d_normalize, its backward a launch of its own)
   median of 3 blocks of 5 steps each; the two routes' gradients compared.
--kernel-only: 1. only, no step timing (for a rocprofv3 --kernel-trace --stats run of its own).  One JSON line per measurement."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cspn_amd  # noqa: E402
from cspn_amd.train_utils import guidance_heads  # noqa: E402


def median_of_blocks(fn, per_block, blocks=3, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    res = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(per_block):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / per_block)
    return statistics.median(res), res


def bench_kernel():
    B, H, W = 64, 304, 1216
    gen = torch.Generator(device="cuda").manual_seed(1)
    g = torch.randn(B, 8, H, W, generator=gen, device="cuda")
    R = torch.randn(B, 8, H, W, generator=gen, device="cuda")
    out = torch.empty_like(g)
    f = cspn_amd._lib.late_symbol("cspn2d_normalize_backward_f32")
    st = torch.cuda.current_stream().cuda_stream
    for norm, nid in (("8sum", 0), ("8sum_abs", 1)):
        def run():
            assert f(g.data_ptr(), R.data_ptr(), out.data_ptr(), B, H, W, nid, st) == 0
        ms, blocks = median_of_blocks(run, 20)
        nbytes = 96 * B * H * W
        print(json.dumps({"what": "cspn2d_normalize_backward_f32", "shape": [B, 8, H, W], "norm": norm, "ms": round(ms, 4),
                          "blocks_ms": [round(v, 4) for v in blocks], "bytes": nbytes, "TBps": round(nbytes / ms / 1e9, 3),
                          "bar_ms": 0.45, "meets_bar": ms <= 0.45}), flush=True)


def bench_steps():
    C, h, w, N = 64, 152, 608, 24
    H, W = 2 * h, 2 * w
    for B in (8, 64):
        gen = torch.Generator(device="cuda").manual_seed(21)
        x = torch.randn(B, C, h, w, generator=gen, device="cuda")
        w6 = torch.randn(8, C, 3, 3, generator=gen, device="cuda") / 24
        w5 = torch.randn(1, C, 3, 3, generator=gen, device="cuda") / 24 + 0.02
        sp = (torch.rand(B, 1, H, W, generator=gen, device="cuda") < 500.0 / (H * W)).float() * 5.0
        go = torch.randn(B, 1, H, W, generator=gen, device="cuda") / (B * H * W)
        prop = cspn_amd.Affinity_Propagate(N, 3, "8sum")
        routes = {
            "raw": lambda xa, wa, wb: prop(*guidance_heads(xa, wa, wb), sp),
            "prenorm": lambda xa, wa, wb: cspn_amd.propagate_prenorm(*guidance_heads(xa, wa, wb, 0, 0, "8sum"), sp, N),
        }
        row, grads = {"what": "training step", "B": B, "x": [B, C, h, w], "n_iter": N}, {}
        for name, route in routes.items():
            xa, wa, wb = (t.clone().requires_grad_(True) for t in (x, w6, w5))

            def step():
                xa.grad = wa.grad = wb.grad = None
                (route(xa, wa, wb) * go).sum().backward()
            ms, blocks = median_of_blocks(step, 5, warm=2)
            row[name + "_ms"], row[name + "_blocks_ms"] = round(ms, 3), [round(v, 3) for v in blocks]
            grads[name] = (xa.grad.clone(), wa.grad.clone(), wb.grad.clone())
            del xa, wa, wb
            torch.cuda.empty_cache()
        for i, k in enumerate(("x", "w6", "w5")):
            a, b = grads["prenorm"][i], grads["raw"][i]
            row["grad_rel_err_" + k] = float((a - b).abs().max() / b.abs().max())
        row["faster"] = "raw" if row["raw_ms"] < row["prenorm_ms"] else "prenorm"
        print(json.dumps(row), flush=True)
        del x, grads
        torch.cuda.empty_cache()


def bench_fused_vs_grad():
    """gate_wb from the training route (raw heads + cspn2d_normalize) against the fused grad-off head: bitwise?"""
    C, h, w = 64, 152, 608
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(2, C, h, w, generator=gen, device="cuda")
    w6 = torch.randn(8, C, 3, 3, generator=gen, device="cuda") / 24
    w5 = torch.randn(1, C, 3, 3, generator=gen, device="cuda") / 24
    for norm in ("8sum", "8sum_abs"):
        with torch.no_grad():
            g0, _ = guidance_heads(x, w6, w5, 0, 0, norm)
        g1, _ = guidance_heads(x.clone().requires_grad_(True), w6, w5, 0, 0, norm)
        g1 = g1.detach()
        print(json.dumps({"what": "gate_wb grad-on vs fused grad-off", "norm": norm, "bitwise": bool(torch.equal(g0.view(torch.int32), g1.view(torch.int32))),
                          "rel_err": float((g0 - g1).abs().max() / g0.abs().max()), "elements_differing": int((g0 != g1).sum())}), flush=True)


if __name__ == "__main__":
    bench_kernel()
    if "--kernel-only" not in sys.argv:
        bench_fused_vs_grad()
        bench_steps()
