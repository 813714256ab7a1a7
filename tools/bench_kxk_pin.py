"""K x K propagation pinned to the measured depth with a per-pixel confidence (cspn2d_forward_kxk_norm_pin / cspn2d_backward_kxk_norm_pin;
K = 3, 5 and 7, dilation 1 and 2, float32 and bfloat16 guidance) beside
  * the unpinned contract of the same build (cspn2d_forward_kxk_norm / cspn2d_backward_kxk_norm: the hard pin to blur_depth), whose kernels are
    the parent commit's instruction for instruction; only the fold and its adjoint differ between the two, and
  * what a port of a CSPN++ / PENet refinement ran before: n_iter one-step Affinity_PropagateKxK(1, K, norm, dilation) calls without a mask with
    the blend (1 - m) x + m sparse in torch between them, under autograd for the training case; time and peak memory.
Shape KITTI x 8 (B 8, 304 x 1216), n_iter 24, C 1, a [B,1] sparse mask of ~500 points per image, pin_conf uniform in [0, 1).  Forward alone and
a training step (the forward that keeps its history, then the backward: gradients of guidance and blur_depth, for the pinned call also of
sparse_depth and pin_conf).  The engine calls are timed in alternating blocks; every time is the median of the prewarmed blocks of event-timed
calls, min / max over the blocks are the spread within the run.  The loop is timed, not compared: a one-step call takes the current level as
its blur_depth, so its (1 - sum_k wb_k) term carries that level where the contract carries H_0; it is the cheapest thing a port can write with
the unpinned modules, a faithful one costs more.  The pinned call is compared at the timed size with the float32 torch statement of the contract
(the reference's padded loop with the blend line, under autograd), float32 guidance.
    python tools/bench_kxk_pin.py [--reps 3] [--blocks 3] [--K 3 5 7] [--D 1 2] [--dtypes float32 bfloat16] [--json out.jsonl] [--no-loop] [--no-check]"""
import argparse
import json
import os
import sys

import torch


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


def peak_mib(f):
    """peak bytes allocated by one call of f above what is allocated before it, in MiB"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def torch_kxk_norm_pin(guidance, blur, sparse, pin, K, n, norm, D):
    c = (K // 2) * D
    P = [(l * D, (K - 1 - l) * D, t * D, (K - 1 - t) * D) for t in range(K) for l in range(K) if (t, l) != (K // 2, K // 2)]
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([torch.nn.functional.pad(g[:, k], P[k]) for k in range(len(P))], 1)
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, c:-c, c:-c]
    gate = gate.unsqueeze(2)
    m = sparse.sign() * pin
    x = blur
    for _ in range(n):
        xp = torch.stack([torch.nn.functional.pad(x, P[k]) for k in range(len(P))], 1)
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, c:-c, c:-c]
        x = (1 - m) * x + m * sparse
    return x


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--K", type=int, nargs="+", default=[3, 5, 7])
    ap.add_argument("--D", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-loop", action="store_true", help="the engine calls only")
    ap.add_argument("--no-check", action="store_true", help="no comparison with the torch statement")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import cspn_amd
    from cspn_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_kxk_pin.py measures on the GPU; none found")
    rows = []
    n, norm, C = 24, "8sum", 1
    B, H, W = 8, 304, 1216
    for K in a.K:
        gen = torch.Generator(device="cuda").manual_seed(K * 10 + C)
        g32 = torch.randn(B, K * K - 1, H, W, device="cuda", generator=gen)
        x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
        s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 500 / (H * W)).float() * (x[:, :1] + 0.1)
        p = torch.rand(B, 1, H, W, device="cuda", generator=gen)
        go = torch.randn(B, C, H, W, device="cuda", generator=gen)
        for D in a.D:
            for dtype in a.dtypes:
                g = g32.to(getattr(torch, dtype))
                row = dict(shape="kitti_x8", B=B, H=H, W=W, K=K, C=C, n_iter=n, norm=norm, dilation=D, guidance=dtype)
                state = {}

                def hard_train():
                    out, hist = F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm, return_history=True, dilation=D)
                    state["hard"] = F.cspn2d_backward_kxk_norm(g, x, s, go, K, n, norm, hist, dilation=D)

                def pin_train():
                    out, hist = F.cspn2d_forward_kxk_norm_pin(g, x, s, p, K, n, norm, return_history=True, dilation=D)
                    state["pin"] = F.cspn2d_backward_kxk_norm_pin(g, x, s, p, go, K, n, norm, hist, dilation=D)
                tf = blocks_of({"hard": lambda: F.cspn2d_forward_kxk_norm(g, x, s, K, n, norm, dilation=D),
                                "pin": lambda: F.cspn2d_forward_kxk_norm_pin(g, x, s, p, K, n, norm, dilation=D)}, a.reps, a.blocks)
                tb = blocks_of({"hard": hard_train, "pin": pin_train}, a.reps, a.blocks)
                row.update(hard_fwd=stats(tf["hard"]), pin_fwd=stats(tf["pin"]), hard_train=stats(tb["hard"]), pin_train=stats(tb["pin"]))
                row.update(pin_over_hard_fwd=round(row["pin_fwd"]["ms"] / row["hard_fwd"]["ms"], 3),
                           pin_over_hard_train=round(row["pin_train"]["ms"] / row["hard_train"]["ms"], 3),
                           pin_fwd_mib=peak_mib(lambda: F.cspn2d_forward_kxk_norm_pin(g, x, s, p, K, n, norm, dilation=D)), pin_train_mib=peak_mib(pin_train))
                if not a.no_loop:
                    step = cspn_amd.Affinity_PropagateKxK(1, K, norm, dilation=D)

                    def loop(gl, xl, pl):
                        ml = s.sign() * pl
                        y = xl
                        for _ in range(n):
                            y = (1 - ml) * step(gl, y) + ml * s
                        return y
                    gl, xl, pl = g.clone().requires_grad_(True), x.clone().requires_grad_(True), p.clone().requires_grad_(True)

                    def loop_fwd():
                        with torch.no_grad():
                            loop(g, x, p)

                    def loop_train():
                        gl.grad = xl.grad = pl.grad = None
                        loop(gl, xl, pl).backward(go)
                    lf = blocks_of({"loop": loop_fwd}, 1, a.blocks)["loop"]
                    lb = blocks_of({"loop": loop_train}, 1, a.blocks)["loop"]
                    row.update(loop_fwd=stats(lf), loop_train=stats(lb), loop_over_pin_fwd=round(lf[len(lf) // 2] / row["pin_fwd"]["ms"], 2),
                               loop_over_pin_train=round(lb[len(lb) // 2] / row["pin_train"]["ms"], 2), loop_fwd_mib=peak_mib(loop_fwd),
                               loop_train_mib=peak_mib(loop_train))
                    del gl, xl, pl
                if dtype == "float32" and not a.no_check:
                    leaves = [t.clone().requires_grad_(True) for t in (g, x, s, p)]
                    ref = torch_kxk_norm_pin(*leaves, K, n, norm, D)
                    ref.backward(go)
                    out = F.cspn2d_forward_kxk_norm_pin(g, x, s, p, K, n, norm, dilation=D)
                    row.update(rel_err_out=rel(out, ref.detach()),
                               **{"rel_err_" + k: rel(t, l.grad) for k, t, l in zip(("dguidance", "dblur", "dsparse", "dpin"), state["pin"], leaves)})
                    del leaves, ref
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
