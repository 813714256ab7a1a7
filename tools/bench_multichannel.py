"""C channels on shared 2D guidance: one multi-channel engine call against C single-channel calls (tests/test_multichannel.py
holds them to the same results).  Forward at KITTI 304 x 1216, B in {8, 64}, C in {1, 2, 4}, with and without a mask; the training
step (history forward + backward) at B = 8, C in {2, 4}.  Every number is the median of 5 prewarmed blocks of event-timed calls.
    python tools/bench_multichannel.py [--reps 20] [--json out.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cspn_amd import functional as F  # noqa: E402

H, W = 304, 1216


def timed(fn, reps, blocks=5):
    for _ in range(3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-forward", action="store_true", help="the B = 8, C = 4 forward only (profiling runs)")
    a = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    rows = []

    def rec(**kw):
        kw["speedup"] = round(kw["loop_ms"] / kw["multi_ms"], 3)
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    shapes = [(8, 4, False)] if a.only_forward else [(B, C, sp) for B in (8, 64) for C in (1, 2, 4) for sp in (False, True)]
    for B, C, sp in shapes:
        g = torch.randn(B, 8, H, W, generator=gen).cuda()
        h = (torch.rand(B, C, H, W, generator=gen) * 10).cuda()
        s = ((torch.rand(B, C, H, W, generator=gen) < 0.01).float() * 5).cuda() if sp else None
        hc = [h[:, c:c + 1].contiguous() for c in range(C)]
        sc = [s[:, c:c + 1].contiguous() for c in range(C)] if sp else [None] * C
        multi = timed(lambda: F.cspn2d_forward_multi(g, h, s, 24), a.reps)
        loop = timed(lambda: [F.cspn2d_forward(g, hc[c], sc[c], 24) for c in range(C)], a.reps)
        rec(what="forward", B=B, C=C, sparse=sp, multi_ms=round(multi, 4), loop_ms=round(loop, 4))
        del g, h, s, hc, sc
        torch.cuda.empty_cache()
    if not a.only_forward:
        for C in (2, 4):
            B = 8
            g = torch.randn(B, 8, H, W, generator=gen).cuda()
            h = (torch.rand(B, C, H, W, generator=gen) * 10).cuda()
            go = torch.randn(B, C, H, W, generator=gen).cuda()
            hc = [h[:, c:c + 1].contiguous() for c in range(C)]
            goc = [go[:, c:c + 1].contiguous() for c in range(C)]

            def step_multi():
                out, hist = F.cspn2d_forward_with_history_multi(g, h, None, 24)
                F.cspn2d_backward_from_history_multi(g, h, None, go, hist, 24)

            def step_loop():
                gg = None
                for c in range(C):
                    out, hist = F.cspn2d_forward_with_history(g, hc[c], None, 24)
                    a_, _ = F.cspn2d_backward_from_history(g, hc[c], None, goc[c], hist, 24)
                    gg = a_ if gg is None else gg + a_

            rec(what="train_step", B=B, C=C, sparse=False, multi_ms=round(timed(step_multi, max(2, a.reps // 4)), 4),
                loop_ms=round(timed(step_loop, max(2, a.reps // 4)), 4))
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
