"""Dilated K x K propagation (cspn2d_forward_kxk_norm / cspn2d_backward_kxk_norm with dilation 2; K = 3, 5 and 7) beside dilation 1 of the
same build and beside the float32 torch statement of the same dilated contract (ZeroPad2d (l D, (K-1-l) D, t D, (K-1-t) D), crop R D; under
autograd for the training case) on the same GPU.  Shape KITTI x 8 (B 8, 304 x 1216), n_iter 24, C 1, a [B,1] sparse mask of ~500 points per
image; forward alone and forward + backward (gradients of guidance and blur_depth).  Outputs and gradients are compared at the timed sizes.
Dilation 2 stages (TH + 2 R D)(TW + 2 R D) / ((TH + 2 R)(TW + 2 R)) times the floats of dilation 1 per 64 x 16 tile and reads the same bytes
from memory otherwise; `staged` in a row is that ratio.  The two dilations are timed in alternating blocks, every time is the median of the
prewarmed blocks of event-timed calls, and min / max over the blocks are the spread within the run.
    python tools/bench_kxk_dilation.py [--reps 5] [--blocks 5] [--K 3 5 7] [--json out.jsonl] [--only-engine]
    python tools/bench_kxk_dilation.py --only-d1 --root DIR    dilation 1 alone, from the package under DIR: a checkout without the keyword
                                                               (the parent commit) runs this way, for the same-code check of the D = 1 kernels"""
import argparse
import json
import os
import sys

import torch

PEAK = 8e12
TH, TW = 16, 64


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
    return dict(ms=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def torch_kxk_norm_dil(guidance, blur, sparse, K, n, norm, D):
    c = (K // 2) * D
    P = [(l * D, (K - 1 - l) * D, t * D, (K - 1 - t) * D) for t in range(K) for l in range(K) if (t, l) != (K // 2, K // 2)]
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([torch.nn.functional.pad(g[:, k], P[k]) for k in range(len(P))], 1)
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, c:-c, c:-c]
    gate = gate.unsqueeze(2)
    m = sparse.sign() if sparse is not None else None
    x = blur
    for _ in range(n):
        xp = torch.stack([torch.nn.functional.pad(x, P[k]) for k in range(len(P))], 1)
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, c:-c, c:-c]
        if m is not None:
            x = (1 - m) * x + m * blur
    return x


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[3, 5, 7])
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-engine", action="store_true", help="no torch statement")
    ap.add_argument("--only-d1", action="store_true", help="dilation 1 alone, called without the keyword")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose cspn_amd is measured")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import cspn_amd  # noqa: F401
    from cspn_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_kxk_dilation.py measures on the GPU; none found")
    rows = []
    n, norm, C = 24, "8sum", 1
    B, H, W = 8, 304, 1216
    for K in a.K:
        KK, R = K * K - 1, K // 2
        gen = torch.Generator(device="cuda").manual_seed(K * 10 + C)
        g = torch.randn(B, KK, H, W, device="cuda", generator=gen)
        x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
        s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 500 / (H * W)).float() * (x[:, :1] + 0.1)
        go = torch.randn(B, C, H, W, device="cuda", generator=gen)
        px = B * H * W
        fwd_bytes = n * px * (4 * KK + 12 * C) + px * (8 * KK + 8 * C + 4)
        row = dict(shape="kitti_x8", root=os.path.basename(os.path.abspath(a.root)), B=B, H=H, W=W, K=K, C=C, n_iter=n, norm=norm,
                   staged=round((TH + 4 * R) * (TW + 4 * R) / ((TH + 2 * R) * (TW + 2 * R)), 3))
        kw = {1: {}} if a.only_d1 else {1: {}, 2: dict(dilation=2)}
        state = {}

        def fwd(D):
            return lambda: F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm, **kw[D])

        def train(D):
            def f():
                out, hist = F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm, return_history=True, **kw[D])
                state[D] = F.cspn2d_backward_kxk_norm(g, x, s, go, K, n, norm, hist, **kw[D])
            return f
        tf = blocks_of({D: fwd(D) for D in kw}, a.reps, a.blocks)
        tb = blocks_of({D: train(D) for D in kw}, a.reps, a.blocks)
        for D in kw:
            row["d%d_fwd" % D], row["d%d_fwd_bw" % D] = stats(tf[D]), stats(tb[D])
            row["d%d_fwd_roofline" % D] = round(fwd_bytes / (row["d%d_fwd" % D]["ms"] * 1e-3) / PEAK, 3)
        if 2 in kw:
            row.update(d2_over_d1_fwd=round(row["d2_fwd"]["ms"] / row["d1_fwd"]["ms"], 3),
                       d2_over_d1_fwd_bw=round(row["d2_fwd_bw"]["ms"] / row["d1_fwd_bw"]["ms"], 3))
        if 2 in kw and not a.only_engine:
            with torch.no_grad():
                t_tf = blocks_of({"t": lambda: torch_kxk_norm_dil(g, x, s, K, n, norm, 2)}, 1, 3)["t"]
                ref = torch_kxk_norm_dil(g, x, s, K, n, norm, 2)
            out = F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm, dilation=2)
            gt, xt = g.clone().requires_grad_(True), x.clone().requires_grad_(True)

            def torch_train():
                gt.grad = xt.grad = None
                torch_kxk_norm_dil(gt, xt, s, K, n, norm, 2).backward(go)
            t_tfb = blocks_of({"t": torch_train}, 1, 3)["t"]
            gg, gx = state[2]
            row.update(torch_d2_fwd=stats(t_tf), torch_d2_fwd_bw=stats(t_tfb), d2_fwd_speedup=round(t_tf[1] / row["d2_fwd"]["ms"], 2),
                       d2_fwd_bw_speedup=round(t_tfb[1] / row["d2_fwd_bw"]["ms"], 2), rel_err_out=rel(out, ref), rel_err_dguidance=rel(gg, gt.grad),
                       rel_err_dblur=rel(gx, xt.grad))
            del gt, xt, ref
        state.clear()
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
