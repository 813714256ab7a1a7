"""The demo's module (reference cspn_paddle/demo.py:20-54) two ways: the port as it stands without this module -- torch abs / sum / div per
channel, then cspn_amd.affinity_propagate -- against cspn_amd.CSPN.cspn (3D: the normalisation inside the persistent kernel; 2D: the HIP
normaliser, then the NONE op).  Forward, and forward + backward (grad of guide and feat), at config 5 (N 4, C 1, 32 x 160 x 608, 12 steps),
at the demo's own sizes (N 3, 48 x 64 x 128, 24 steps, C 1 and 3) and in 2D at KITTI x 8 (N 8, 304 x 1216, 24 steps).  Also the stand-alone
normaliser and its adjoint at config 5, priced at 2 K 4 / 3 K 4 B per voxel.  Every number is the median of 5 prewarmed blocks of
event-timed calls.
    python tools/bench_absnorm.py [--reps 10] [--json out.jsonl] [--only-config5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cspn_amd  # noqa: E402
from cspn_amd import functional as F  # noqa: E402


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


def port_today(guide, feat, n_iter):
    K = 3 ** (feat.dim() - 2) - 1
    outs = []
    for c in range(feat.shape[1]):
        s = guide[:, c * K:(c + 1) * K].abs()
        outs.append(cspn_amd.affinity_propagate(feat[:, c:c + 1], s / s.sum(1, keepdim=True), 3, n_iter))
    return outs[0] if len(outs) == 1 else torch.cat(outs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-config5", action="store_true", help="the config-5 forward only (profiling runs)")
    a = ap.parse_args()
    rows = []

    def rec(**kw):
        if "today_ms" in kw:
            kw["speedup"] = round(kw["today_ms"] / kw["cspn_ms"], 3)
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    cases = [("config5", 4, 1, (32, 160, 608), 12)]
    if not a.only_config5:
        cases += [("demo_c1", 3, 1, (48, 64, 128), 24), ("demo_c3", 3, 3, (48, 64, 128), 24), ("kitti_x8_2d", 8, 1, (304, 1216), 24)]
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, N, C, S, n in cases:
        d = len(S)
        K = 3 ** d - 1
        m = cspn_amd.CSPN(d, C, 3, n)
        g = torch.rand(N, C * K, *S, device="cuda", generator=gen) - 0.2
        x = torch.rand(N, C, *S, device="cuda", generator=gen)
        reps = max(2, a.reps // (4 if name == "config5" else 1))
        with torch.no_grad():
            today = timed(lambda: port_today(g, x, n), reps)
            new = timed(lambda: m.cspn(g, x), reps)
        rec(what="forward", case=name, N=N, C=C, S=list(S), n_iter=n, today_ms=round(today, 4), cspn_ms=round(new, 4))
        if a.only_config5:
            break
        go = torch.randn(N, C, *S, device="cuda", generator=gen)
        gr, xr = g.clone().requires_grad_(True), x.clone().requires_grad_(True)

        def step(fn):
            gr.grad = xr.grad = None
            fn(gr, xr, n).backward(go)

        today = timed(lambda: step(port_today), max(2, reps // 2))
        new = timed(lambda: step(lambda gg, xx, nn: m.cspn(gg, xx)), max(2, reps // 2))
        rec(what="forward+backward", case=name, N=N, C=C, S=list(S), n_iter=n, today_ms=round(today, 4), cspn_ms=round(new, 4))
        if name == "config5":
            V = N * C
            for s_ in S:
                V *= s_
            gw = torch.randn_like(g)
            fwd = timed(lambda: F._gate_absnorm(g, K), reps)
            bwd = timed(lambda: F.gate_absnorm_backward(g, gw, K), reps)
            del gw
            rec(what="normaliser", case=name, K=K, voxels=V, ms=round(fwd, 4), tbps=round(2 * K * 4 * V / fwd / 1e9, 3))
            rec(what="normaliser_backward", case=name, K=K, voxels=V, ms=round(bwd, 4), tbps=round(3 * K * 4 * V / bwd / 1e9, 3))
        del g, x, go, gr, xr
        torch.cuda.empty_cache()
    cspn_amd.cspn3d_check_status()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
