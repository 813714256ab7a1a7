"""The depth-completion contract over K x K (cspn2d_forward_kxk_norm / cspn2d_backward_kxk_norm, K = 5 and 7) against the float32 torch
statement of the same contract (the reference's padded normalisation and loop, cspn.py:42-144, with the ZeroPad2d tuples generalised to
K x K; under autograd for the training case) on the same GPU.  Shape KITTI x 8 (B 8, 304 x 1216), n_iter 24, C 1 and 2, a [B,1] sparse
mask of ~500 points per image; forward alone and forward + backward (gradients of guidance and blur_depth).  Outputs and gradients are
compared at the timed sizes.  Fraction of the 8 TB/s roofline from the algorithmic bytes per pixel:
    forward step       4 KK + 12 C        (w', then H read, H written and b read), KK = K*K - 1
    fold               8 KK + 8 C + 4     (once per call: guidance and w', blur and b, the mask)
    forward            n (4 KK + 12 C) + 8 KK + 8 C + 4
Every time is the median of 5 prewarmed blocks of event-timed calls.
    python tools/bench_kxk_norm.py [--reps 5] [--K 5 7] [--C 1 2] [--json out.jsonl] [--only-engine]"""
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


def torch_kxk_norm(guidance, blur, sparse, K, n, norm):
    """the torch statement: gates padded with ZeroPad2d((l, K-1-l, t, K-1-t)), normalised by their abs-sum, the depth padded the same
    way, the weighted sum cropped by R, plus (1 - gate_sum) blur, sparse depth pinned"""
    R = K // 2
    P = [(l, K - 1 - l, t, K - 1 - t) for t in range(K) for l in range(K) if (t, l) != (R, R)]
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([torch.nn.functional.pad(g[:, k], P[k]) for k in range(len(P))], 1)
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, R:-R, R:-R]
    gate = gate.unsqueeze(2)
    m = sparse.sign() if sparse is not None else None
    x = blur
    for _ in range(n):
        xp = torch.stack([torch.nn.functional.pad(x, P[k]) for k in range(len(P))], 1)
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, R:-R, R:-R]
        if m is not None:
            x = (1 - m) * x + m * blur
    return x


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--C", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-engine", action="store_true", help="the engine's calls only (profiling runs)")
    a = ap.parse_args()
    rows = []
    n, norm = 24, "8sum"
    B, H, W = 8, 304, 1216
    for K in a.K:
        for C in a.C:
            KK = K * K - 1
            gen = torch.Generator(device="cuda").manual_seed(K * 10 + C)
            g = torch.randn(B, KK, H, W, device="cuda", generator=gen)
            x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
            s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 500 / (H * W)).float() * (x[:, :1] + 0.1)
            go = torch.randn(B, C, H, W, device="cuda", generator=gen)
            px = B * H * W
            step_bytes = px * (4 * KK + 12 * C)
            fwd_bytes = n * step_bytes + px * (8 * KK + 8 * C + 4)
            row = dict(shape="kitti_x8", B=B, H=H, W=W, K=K, C=C, n_iter=n, norm=norm, guidance_MB=round(4 * KK * px / 1e6, 1))
            t_f = timed(lambda: F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm), a.reps)
            state = {}

            def train():
                out, hist = F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm, return_history=True)
                state["grads"] = F.cspn2d_backward_kxk_norm(g, x, s, go, K, n, norm, hist)
            t_fb = timed(train, a.reps)
            row.update(engine_fwd_ms=round(t_f, 3), engine_fwd_bw_ms=round(t_fb, 3), fwd_TBps=round(fwd_bytes / (t_f * 1e-3) / 1e12, 2),
                       fwd_roofline=round(fwd_bytes / (t_f * 1e-3) / PEAK, 3), step_bytes_per_px=4 * KK + 12 * C)
            if not a.only_engine:
                with torch.no_grad():
                    t_tf = timed(lambda: torch_kxk_norm(g, x, s, K, n, norm), 1, blocks=3)
                    ref = torch_kxk_norm(g, x, s, K, n, norm)
                out = F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm)
                gt, xt = g.clone().requires_grad_(True), x.clone().requires_grad_(True)

                def torch_train():
                    gt.grad = xt.grad = None
                    torch_kxk_norm(gt, xt, s, K, n, norm).backward(go)
                t_tfb = timed(torch_train, 1, blocks=3)
                gg, gx = state["grads"]
                row.update(torch_fwd_ms=round(t_tf, 3), torch_fwd_bw_ms=round(t_tfb, 3), fwd_speedup=round(t_tf / t_f, 2),
                           fwd_bw_speedup=round(t_tfb / t_fb, 2), rel_err_out=rel(out, ref), rel_err_dguidance=rel(gg, gt.grad),
                           rel_err_dblur=rel(gx, xt.grad))
                del gt, xt, ref
            del state
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
