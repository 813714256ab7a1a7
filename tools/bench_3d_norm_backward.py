"""One training step (forward + backward) of the 3D depth-completion contract at config 5's volume (4 x 26 x 32 x 160 x 608), n_iter 12,
'8sum_abs', without a mask and with 5 % of the voxels pinned, in one process on one GPU:
    engine  cspn_amd.Affinity_Propagate3d: cspn3d_forward_f32 + cspn3d_backward_norm_f32 (algo 'auto', and 'stepwise' for information)
    torch   autograd through the float32 plain-torch statement of the same equations (pad + shifted slices), same inputs
A time is the median of event-timed blocks after a warm-up (min and max are printed next to it).  Also: the workspace sizes, and the
max-norm difference of the two routes' gradients at the timed size.
    python tools/bench_3d_norm_backward.py [--json out.json] [--shape B D H W] [--n-iter 12]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cspn_amd  # noqa: E402
from cspn_amd import _lib  # noqa: E402
from oracle.backward import OFF3  # noqa: E402


def statement(g, feat, sparse, n_iter, norm):
    """the forward of include/cspn_amd.h's cspn3d_backward_norm_f32 comment in plain torch ops (tests/test_backward3d_norm.py pins it to
    the oracle)"""
    D, H, W = g.shape[2:]

    def shift(a, off):
        dz, dy, dx = off
        pad = torch.nn.functional.pad(a, (1, 1, 1, 1, 1, 1))
        return pad[:, 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    h0 = feat[:, 0]
    gt = g.abs() if norm == "8sum_abs" else g
    G = [shift(gt[:, k], OFF3[k]) for k in range(26)]
    S = sum(x.abs() for x in G)
    wb = [x / S for x in G]
    m = torch.sign(sparse[:, 0]) if sparse is not None else torch.zeros_like(h0)
    u = 1 - m
    w = [u * x for x in wb]
    c = (u * (1 - sum(wb)) + m) * h0
    x = h0
    for _ in range(n_iter):
        x = c + sum(w[k] * shift(x, OFF3[k]) for k in range(26))
    return x[:, None]


def timed(fn, warm, blocks, reps):
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
    ap.add_argument("--json", default=None)
    ap.add_argument("--shape", type=int, nargs=4, default=(4, 32, 160, 608), metavar=("B", "D", "H", "W"))
    ap.add_argument("--n-iter", type=int, default=12)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    (B, D, H, W), N, norm = a.shape, a.n_iter, "8sum_abs"
    gen = torch.Generator(device="cuda").manual_seed(0)
    g = torch.rand(B, 26, D, H, W, generator=gen, device="cuda") - 0.3
    feat = torch.rand(B, 1, D, H, W, generator=gen, device="cuda")
    go = torch.randn(B, 1, D, H, W, generator=gen, device="cuda")
    sparse5 = (torch.rand(B, 1, D, H, W, generator=gen, device="cuda") < 0.05).float() * (feat + 0.1)
    module = cspn_amd.Affinity_Propagate3d(N, 3, norm)

    def step(route, sp):
        g1, f1 = g.detach().requires_grad_(True), feat.detach().requires_grad_(True)
        if route == "torch":
            out = statement(g1, f1, sp, N, norm)
        else:
            module.algo = route
            out = module(g1, f1, sp)
        out.backward(go)
        return g1.grad, f1.grad

    query = _lib.symbol("cspn3d_backward_norm_workspace_bytes")
    res = {"shape": [B, D, H, W], "n_iter": N, "norm_type": norm,
           "workspace_bytes_backward": query(B, D, H, W, N, _lib.NORM_TYPES[norm], 1),
           "workspace_bytes_forward": _lib.symbol("cspn3d_workspace_bytes_ex")(B, D, H, W, N, _lib.NORM_TYPES[norm], 1)}
    for name, sp in (("no_mask", None), ("mask_5pct", sparse5)):
        eg, ef = step("auto", sp)
        tg, tf = step("torch", sp)
        cspn_amd.cspn3d_check_status()
        row = {"max_norm_diff_engine_vs_torch": {"grad_guidance": float((eg - tg).abs().max() / tg.abs().max()),
                                                 "grad_feat": float((ef - tf).abs().max() / tf.abs().max())}}
        del eg, ef, tg, tf
        row["engine_auto"] = timed(lambda: step("auto", sp), 3, 7, 5)
        row["engine_stepwise"] = timed(lambda: step("stepwise", sp), 3, 7, 5)
        row["torch_autograd"] = timed(lambda: step("torch", sp), 1, 5, 1)
        cspn_amd.cspn3d_check_status()
        row["torch_over_engine"] = row["torch_autograd"]["median_ms"] / row["engine_auto"]["median_ms"]
        res[name] = row
        print(name, json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
