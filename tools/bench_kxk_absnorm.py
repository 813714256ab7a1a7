"""The demo module's route through the K x K engine (cspn2d_forward_kxk_absnorm / cspn2d_backward_kxk_absnorm: the gates normalised
inside the step) against the composed route it replaces, in the same process on the same GPU:
    composed   gate_absnorm -> cspn2d_forward_kxk (history kept) -> cspn2d_backward_kxk -> gate_absnorm_backward, with guide.float()
               in front for a 16-bit guide (the gate normaliser is float32 only)
    fused      the two new calls on the raw guide
The guide is [N * C, KK, H, W] and the values [N * C, 1, H, W]: the folded views CSPN(2, C, K, n) hands over.  KITTI x 8 (N 8,
304 x 1216), n_iter 24, K 5 and 7, C (feat_chan) 1 and 4, float32 / float16 / bfloat16.  The two routes alternate within a round and the
rounds repeat; a time is the median over the rounds of the per-round median of --reps prewarmed event-timed blocks, and "spread" is
(max - min) / median of the composed route over the rounds: the yardstick for "faster" and "not slower".  Peak memory is
max_memory_allocated over one call less what was allocated before it.  Roofline fractions use each route's own algorithmic bytes per
pixel for the forward over 8 TB/s, with e the guide's element size:
    composed   (e + 4) KK [+ (2 + 4) KK for the cast] + n (4 KK + 8)
    fused      n (e KK + 8)
    python tools/bench_kxk_absnorm.py [--reps 5] [--rounds 3] [--json out.jsonl] [--shape N H W] [--K 5 7] [--C 1 4]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cspn_amd  # noqa: E402,F401
from cspn_amd import functional as F  # noqa: E402
from tools.bench_kxk import PEAK, timed  # noqa: E402


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    del r
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--shape", type=int, nargs=3, default=(8, 304, 1216), metavar=("N", "H", "W"))
    ap.add_argument("--K", type=int, nargs="+", default=(5, 7))
    ap.add_argument("--C", type=int, nargs="+", default=(1, 4))
    ap.add_argument("--dtypes", nargs="+", default=("float32", "float16", "bfloat16"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    N, H, W = a.shape
    n = 24
    rows = []
    for K in a.K:
        KK = K * K - 1
        for C in a.C:
            for name in a.dtypes:
                dtype = getattr(torch, name)
                gen = torch.Generator(device="cuda").manual_seed(K * 10 + C)
                M = N * C
                g = ((torch.rand(M, KK, H, W, device="cuda", generator=gen) + 0.05)
                     * (torch.rand(M, KK, H, W, device="cuda", generator=gen) < 0.5).float().mul_(2).sub_(1)).to(dtype)
                x = torch.rand(M, 1, H, W, device="cuda", generator=gen)
                go = torch.randn(M, 1, H, W, device="cuda", generator=gen)
                px = M * H * W
                e = g.element_size()

                def composed_fwd():
                    return F.cspn2d_forward_kxk(F.gate_absnorm(g.float(), KK), x, K, n)

                def composed_fb():
                    g32 = g.float()
                    w = F.gate_absnorm(g32, KK)
                    out, hist = F.cspn2d_forward_kxk(w, x, K, n, return_history=True)
                    w = F.gate_absnorm(g32, KK)   # the parent's backward recomputes it
                    gw, gx = F.cspn2d_backward_kxk(w, x, go, K, n, hist)
                    return out, F.gate_absnorm_backward(g32, gw, KK).to(dtype), gx

                def fused_fwd():
                    return F.cspn2d_forward_kxk_absnorm(g, x, K, n)

                def fused_fb():
                    out, hist = F.cspn2d_forward_kxk_absnorm(g, x, K, n, return_history=True)
                    return (out,) + F.cspn2d_backward_kxk_absnorm(g, x, go, K, n, hist)

                variants = {"composed_fwd": composed_fwd, "fused_fwd": fused_fwd, "composed_fb": composed_fb, "fused_fb": fused_fb}
                ts = {k: [] for k in variants}
                for _ in range(a.rounds):
                    for k, fn in variants.items():
                        ts[k].append(timed(fn, a.reps))
                t = {k: med(v) for k, v in ts.items()}
                spread = {k: (max(v) - min(v)) / t[k] for k, v in ts.items()}
                mem = {k: peak_bytes(fn) for k, fn in variants.items()}
                ref, got = composed_fwd(), fused_fwd()
                err = float((ref - got).abs().max() / ref.abs().max())
                b_comp = px * ((e + 4) * KK + (6 * KK if e == 2 else 0) + n * (4 * KK + 8))
                b_fused = px * n * (e * KK + 8)
                row = dict(N=N, C=C, H=H, W=W, K=K, dtype=name, n_iter=n, rounds=a.rounds, reps=a.reps,
                           composed_fwd_ms=round(t["composed_fwd"], 3), fused_fwd_ms=round(t["fused_fwd"], 3),
                           composed_fb_ms=round(t["composed_fb"], 3), fused_fb_ms=round(t["fused_fb"], 3),
                           composed_fwd_spread=round(spread["composed_fwd"], 4), composed_fb_spread=round(spread["composed_fb"], 4),
                           fused_fwd_spread=round(spread["fused_fwd"], 4), fused_fb_spread=round(spread["fused_fb"], 4),
                           fwd_speedup=round(t["composed_fwd"] / t["fused_fwd"], 3), fb_speedup=round(t["composed_fb"] / t["fused_fb"], 3),
                           composed_fwd_roofline=round(b_comp / (t["composed_fwd"] * 1e-3) / PEAK, 3),
                           fused_fwd_roofline=round(b_fused / (t["fused_fwd"] * 1e-3) / PEAK, 3),
                           composed_fwd_peak_mb=round(mem["composed_fwd"] / 2 ** 20, 1), fused_fwd_peak_mb=round(mem["fused_fwd"] / 2 ** 20, 1),
                           composed_fb_peak_mb=round(mem["composed_fb"] / 2 ** 20, 1), fused_fb_peak_mb=round(mem["fused_fb"] / 2 ** 20, 1),
                           fwd_max_rel_diff=err)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del g, x, go, ref, got
                torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
