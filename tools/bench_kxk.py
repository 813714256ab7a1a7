"""The 2D K x K engine (cspn2d_forward_kxk / cspn2d_backward_kxk, K = 5 and 7) against the float32 torch statement of the same recurrence
(pad, then K*K-1 shifted multiply-adds per step; under autograd for the training case) on the same GPU.  Shapes KITTI x 8 (N 8, 304 x 1216)
and NYU x 16 (N 16, 228 x 304), n_iter 24, C 1 and 2; forward alone and forward + backward (gradients of gate and x).  Outputs and
gradients are compared at the timed sizes.  Fraction of the 8 TB/s roofline from the algorithmic bytes per pixel:
    forward            n (4 (K*K-1) + 8 C)
    forward, training  the same (the kept levels are the steps' own stores)
    backward           n (4 (K*K-1) + 8 C) for the adjoint steps + 8 n C + 4 (K*K-1) for the gate gradient
Every time is the median of 5 prewarmed blocks of event-timed calls.
    python tools/bench_kxk.py [--reps 5] [--json out.jsonl] [--only-engine]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cspn_amd  # noqa: E402,F401
from cspn_amd import functional as F  # noqa: E402

PEAK = 8e12


def timed(fn, reps, blocks=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    ts.sort()
    return ts[len(ts) // 2]


def torch_kxk(g, x, K, n):
    """the float32 torch statement: H_{t+1}(p) = sum_k g_k(p) H_t(p + off_k), zero outside"""
    R = K // 2
    H, W = x.shape[2:]
    offs = [(R - t, R - l) for t in range(K) for l in range(K) if (t, l) != (R, R)]
    for _ in range(n):
        pad = torch.nn.functional.pad(x, (R, R, R, R))
        acc = 0
        for k, (dy, dx) in enumerate(offs):
            acc = acc + g[:, k:k + 1] * pad[:, :, R + dy:R + dy + H, R + dx:R + dx + W]
        x = acc
    return x


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-engine", action="store_true", help="the engine's calls only (profiling runs)")
    a = ap.parse_args()
    rows = []
    n = 24
    for name, N, H, W in (("kitti_x8", 8, 304, 1216), ("nyu_x16", 16, 228, 304)):
        for K in (5, 7):
            for C in (1, 2):
                KK = K * K - 1
                gen = torch.Generator(device="cuda").manual_seed(K * 10 + C)
                g = (torch.randn(N, KK, H, W, device="cuda", generator=gen) * (1.2 / KK))
                x = torch.rand(N, C, H, W, device="cuda", generator=gen)
                go = torch.randn(N, C, H, W, device="cuda", generator=gen)
                px = N * H * W
                fwd_bytes = n * px * (4 * KK + 8 * C)
                bwd_bytes = n * px * (4 * KK + 8 * C) + px * (8 * n * C + 4 * KK)
                row = dict(shape=name, N=N, H=H, W=W, K=K, C=C, n_iter=n, gate_MB=round(4 * KK * px / 1e6, 1))
                # the engine
                t_f = timed(lambda: F.cspn2d_forward_kxk(g, x, K, n), a.reps)
                state = {}

                def train():
                    out, hist = F.cspn2d_forward_kxk(g, x, K, n, return_history=True)
                    state["grads"] = F.cspn2d_backward_kxk(g, x, go, K, n, hist)
                t_fb = timed(train, a.reps)
                _, hist = F.cspn2d_forward_kxk(g, x, K, n, return_history=True)
                t_b = timed(lambda: F.cspn2d_backward_kxk(g, x, go, K, n, hist), a.reps)
                row.update(engine_fwd_ms=round(t_f, 3), engine_fwd_bw_ms=round(t_fb, 3), engine_bwd_ms=round(t_b, 3),
                           fwd_step_us=round(1e3 * t_f / n, 1), fwd_roofline=round(fwd_bytes / (t_f * 1e-3) / PEAK, 3),
                           bwd_roofline=round(bwd_bytes / (t_b * 1e-3) / PEAK, 3), fwd_TBps=round(fwd_bytes / (t_f * 1e-3) / 1e12, 2),
                           bwd_TBps=round(bwd_bytes / (t_b * 1e-3) / 1e12, 2))
                if not a.only_engine:
                    with torch.no_grad():
                        t_tf = timed(lambda: torch_kxk(g, x, K, n), max(1, a.reps // 2), blocks=3)
                        ref = torch_kxk(g, x, K, n)
                    out = F.cspn2d_forward_kxk(g, x, K, n)
                    gt, xt = g.clone().requires_grad_(True), x.clone().requires_grad_(True)

                    def torch_train():
                        gt.grad = xt.grad = None
                        torch_kxk(gt, xt, K, n).backward(go)
                    t_tfb = timed(torch_train, 1, blocks=3)
                    gg, gx = state["grads"]
                    row.update(torch_fwd_ms=round(t_tf, 3), torch_fwd_bw_ms=round(t_tfb, 3), fwd_speedup=round(t_tf / t_f, 2),
                               fwd_bw_speedup=round(t_tfb / t_fb, 2), rel_err_out=rel(out, ref), rel_err_dgate=rel(gg, gt.grad),
                               rel_err_dx=rel(gx, xt.grad))
                    del gt, xt, ref
                del hist, state
                rows.append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
