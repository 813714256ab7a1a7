"""Assembling K x K propagation levels per pixel (cspn2d_forward_kxk_assemble / cspn2d_backward_kxk_assemble, Affinity_PropagateAssemble)
against the two routes a user had before the call existed, on the same GPU in the same process, the two sides of each comparison timed in
alternating blocks:
    inference route   cspn2d_forward_kxk_norm(..., return_history=True), which stores the n - 1 levels, then T torch multiply-adds over them
    training route    T calls of Affinity_PropagateKxK with n_iter = s_j under autograd, the weighted sum in torch, loss.backward()
Shape KITTI x 8 (B 8, 304 x 1216), C 1, n_iter 24, K 3 / 5 / 7, steps (24,) and (6, 12, 18, 24), a [B,1] sparse mask of ~500 points per
image, conf = softmax over the T collected levels.  Forward alone (no autograd) and one training step (forward + backward for the gradients
of guidance, blur_depth and conf; the assembling side through the module, as the route it replaces).  Every time is the median of 5
prewarmed blocks of event-timed calls, with the blocks' minimum and maximum beside it; peak memory is torch's max_memory_allocated over one call
of each route, above what the inputs hold.  Outputs and gradients of the two routes are compared at the timed size.
Algorithmic bytes per pixel of the assembling forward (KK = K*K - 1): n (4 KK + 12 C) + 8 KK + 8 C + 4 for the steps and the fold, less 4 C
for the last level (not stored), plus 4 + 8 C per collected step (4 + 4 C for the first).
    python tools/bench_kxk_assemble.py [--reps 5] [--K 3 5 7] [--json out.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cspn_amd  # noqa: E402
from cspn_amd import functional as F  # noqa: E402

PEAK = 8e12
STEPS = [(24,), (6, 12, 18, 24)]


def timed_pair(fa, fb, reps, blocks=5):
    """-> ((median, min, max) of fa, the same of fb) in ms per call; the blocks of the two alternate"""
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(blocks):
        for i, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) / reps)
    return tuple((sorted(t)[len(t) // 2], min(t), max(t)) for t in ts)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[3, 5, 7])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    n, norm, C = 24, "8sum", 1
    B, H, W = 8, 304, 1216
    px = B * H * W
    for K in a.K:
        KK = K * K - 1
        gen = torch.Generator(device="cuda").manual_seed(K)
        g = torch.randn(B, KK, H, W, device="cuda", generator=gen)
        x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
        s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 500 / (H * W)).float() * (x[:, :1] + 0.1)
        go = torch.randn(B, C, H, W, device="cuda", generator=gen)
        for steps in STEPS:
            T = len(steps)
            conf = torch.softmax(torch.randn(B, T, H, W, device="cuda", generator=gen), 1)
            fwd_bytes = px * (n * (4 * KK + 12 * C) + 8 * KK + 8 * C + 4 - 4 * C + T * (4 + 8 * C) - 4 * C)
            row = dict(shape="kitti_x8", B=B, H=H, W=W, K=K, C=C, n_iter=n, steps=list(steps), norm=norm)

            def assemble_fwd():
                return F.cspn2d_forward_kxk_assemble(g, x, s, conf, steps, K, n, norm)

            def route_fwd():
                out, hist = F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm, return_history=True)
                lv = hist.view(n - 1, B, C, H, W)
                acc = conf[:, T - 1:T] * out
                for j in range(T - 1):
                    acc = torch.addcmul(acc, conf[:, j:j + 1], lv[steps[j] - 1])
                return acc
            with torch.no_grad():
                (tf, tf0, tf1), (rf, rf0, rf1) = timed_pair(assemble_fwd, route_fwd, a.reps)
                row.update(fwd_ms=round(tf, 3), fwd_spread=[round(tf0, 3), round(tf1, 3)], route_fwd_ms=round(rf, 3),
                           route_fwd_spread=[round(rf0, 3), round(rf1, 3)], fwd_speedup=round(rf / tf, 2),
                           fwd_TBps=round(fwd_bytes / (tf * 1e-3) / 1e12, 2), fwd_roofline=round(fwd_bytes / (tf * 1e-3) / PEAK, 3),
                           fwd_peak_MB=round(peak_mb(assemble_fwd), 1), route_fwd_peak_MB=round(peak_mb(route_fwd), 1),
                           rel_err_out=rel(assemble_fwd(), route_fwd()))
            leaves = [t.clone().requires_grad_(True) for t in (g, x, conf)]
            module = cspn_amd.Affinity_PropagateAssemble(n, (K,), steps, norm)
            parts = [cspn_amd.Affinity_PropagateKxK(sj, K, norm) for sj in steps]

            def clear():
                for t in leaves:
                    t.grad = None

            def assemble_train():
                clear()
                module([leaves[0]], leaves[1], s, [leaves[2]]).backward(go)

            def route_train():
                clear()
                out = None
                for j, m in enumerate(parts):
                    y = leaves[2][:, j:j + 1] * m(leaves[0], leaves[1], s)
                    out = y if out is None else out + y
                out.backward(go)
            (tt, tt0, tt1), (rt, rt0, rt1) = timed_pair(assemble_train, route_train, a.reps)
            assemble_train()
            mine = [t.grad.clone() for t in leaves]
            route_train()
            row.update(train_ms=round(tt, 3), train_spread=[round(tt0, 3), round(tt1, 3)], route_train_ms=round(rt, 3),
                       route_train_spread=[round(rt0, 3), round(rt1, 3)], train_speedup=round(rt / tt, 2),
                       train_peak_MB=round(peak_mb(assemble_train), 1), route_train_peak_MB=round(peak_mb(route_train), 1),
                       rel_err_dguidance=rel(mine[0], leaves[0].grad), rel_err_dblur=rel(mine[1], leaves[1].grad),
                       rel_err_dconf=rel(mine[2], leaves[2].grad))
            clear()
            del leaves, mine
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
