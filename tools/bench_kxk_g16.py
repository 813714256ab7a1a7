"""The 2D K x K engine on fp16 / bf16 gates (cspn2d_forward_kxk / cspn2d_backward_kxk -> cspn2d_*_kxk_g16) against its own float32 path
in the same process on the same GPU.  The float32 entry points are untouched by the 16-bit work (their kernels compile to the same code),
so they are the baseline.  KITTI x 8 (N 8, 304 x 1216), n_iter 24, K 5 and 7, C 1 and 4, both 16-bit types.  Per row:
    f32        the float32 path on gates widened outside the timed region
    f32+cast   the float32 path with gate.float() inside the timed region (what a caller of the float32-only engine had to do)
    g16        the 16-bit path
each for the forward alone and for forward + backward (history-keeping forward, then the backward for gate and x).  The variants alternate
within a round and the rounds repeat; a time is the median over the rounds of the per-round median of 5 prewarmed event-timed blocks, and
"spread" is (max - min) / median of the float32 path over the rounds -- the yardstick for "not slower".  Roofline fractions use the
algorithmic bytes per pixel and step over 8 TB/s: float32 4 (K*K-1) + 8 C, 16-bit 2 (K*K-1) + 8 C.  Outputs are compared at the timed size.
    python tools/bench_kxk_g16.py [--reps 5] [--rounds 3] [--json out.jsonl] [--shape N H W] [--K 5 7] [--C 1 4]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--shape", type=int, nargs=3, default=(8, 304, 1216), metavar=("N", "H", "W"),
                    help="W % 4 != 0 times the guarded scalar instances")
    ap.add_argument("--K", type=int, nargs="+", default=(5, 7))
    ap.add_argument("--C", type=int, nargs="+", default=(1, 4))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    N, H, W = a.shape
    n = 24
    rows = []
    for K in a.K:
        KK = K * K - 1
        for C in a.C:
            for dtype in (torch.float16, torch.bfloat16):
                gen = torch.Generator(device="cuda").manual_seed(K * 10 + C)
                g16 = (torch.randn(N, KK, H, W, device="cuda", generator=gen) * (1.2 / KK)).to(dtype)
                g32 = g16.float()
                x = torch.rand(N, C, H, W, device="cuda", generator=gen)
                go = torch.randn(N, C, H, W, device="cuda", generator=gen)
                px = N * H * W

                def train(g):
                    out, hist = F.cspn2d_forward_kxk(g, x, K, n, return_history=True)
                    return F.cspn2d_backward_kxk(g, x, go, K, n, hist)
                variants = {
                    "f32_fwd": lambda: F.cspn2d_forward_kxk(g32, x, K, n),
                    "cast_fwd": lambda: F.cspn2d_forward_kxk(g16.float(), x, K, n),
                    "g16_fwd": lambda: F.cspn2d_forward_kxk(g16, x, K, n),
                    "f32_fb": lambda: train(g32),
                    "cast_fb": lambda: train(g16.float()),
                    "g16_fb": lambda: train(g16),
                }
                ts = {k: [] for k in variants}
                for _ in range(a.rounds):
                    for k, fn in variants.items():
                        ts[k].append(timed(fn, a.reps))
                t = {k: med(v) for k, v in ts.items()}
                same = bool(torch.equal(F.cspn2d_forward_kxk(g16, x, K, n), F.cspn2d_forward_kxk(g32, x, K, n)))
                b32, b16 = n * px * (4 * KK + 8 * C), n * px * (2 * KK + 8 * C)
                row = dict(N=N, H=H, W=W, K=K, C=C, dtype=str(dtype).replace("torch.", ""), n_iter=n, rounds=a.rounds,
                           f32_fwd_ms=round(t["f32_fwd"], 3), cast_fwd_ms=round(t["cast_fwd"], 3), g16_fwd_ms=round(t["g16_fwd"], 3),
                           f32_fb_ms=round(t["f32_fb"], 3), cast_fb_ms=round(t["cast_fb"], 3), g16_fb_ms=round(t["g16_fb"], 3),
                           f32_fwd_spread=round((max(ts["f32_fwd"]) - min(ts["f32_fwd"])) / t["f32_fwd"], 4),
                           g16_fwd_spread=round((max(ts["g16_fwd"]) - min(ts["g16_fwd"])) / t["g16_fwd"], 4),
                           f32_fb_spread=round((max(ts["f32_fb"]) - min(ts["f32_fb"])) / t["f32_fb"], 4),
                           fwd_speedup=round(t["f32_fwd"] / t["g16_fwd"], 3), fwd_speedup_vs_cast=round(t["cast_fwd"] / t["g16_fwd"], 3),
                           fb_speedup=round(t["f32_fb"] / t["g16_fb"], 3), fb_speedup_vs_cast=round(t["cast_fb"] / t["g16_fb"], 3),
                           f32_fwd_roofline=round(b32 / (t["f32_fwd"] * 1e-3) / PEAK, 3),
                           g16_fwd_roofline=round(b16 / (t["g16_fwd"] * 1e-3) / PEAK, 3),
                           g16_fwd_step_us=round(1e3 * t["g16_fwd"] / n, 1), fwd_bitwise_equal=same)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del g16, g32, x, go
                torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
