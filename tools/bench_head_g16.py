"""The 3 x 3 model's guidance heads on a float16 / bfloat16 feature map (train_utils.guidance_heads(..., guidance_dtype=torch.float32): cspn_guidance_head_g16
and its backward, float32 guidance and blur straight off the 16-bit matrix instructions) against the only route a user had before them, on the same GPU in the
same process, in alternating blocks:
  * f32route   x.float() plus the float32 guidance_heads (forward), and guidance_heads_backward on that x.float() plus .to(dt) of dL/dx (backward; the forward's
               x.float() is kept, as autograd keeps it).
Shapes KITTI x 8 and KITTI x 64 (x [B,64,152,608] -> [B,8,304,1216] + [B,1,304,1216]), both dtypes, forward alone and forward + backward (all three
gradients).  Every time is the median of 5 prewarmed blocks of event-timed calls; min and max of the blocks are kept as the spread.
    *_bytes_frac   the call's own bytes / time / 8 TB/s.  Forward: x 2 B per input pixel and channel, guidance + blur 36 B per output pixel.  Backward: both
                   float32 gradients read and written back as dt (54 B per output pixel), the dt planes and x read twice -- dL/dx and dL/dW --, dL/dx written
    *_flop_frac    2 * 9 * C * 9 * B * h * w FLOP (three such GEMMs with the backward) / time / 2.5 PFLOP/s (the 16-bit matrix peak)
    beats_bar      the 16-bit call is faster than the route by more than the two spreads together
--step adds the thing a user feels, at KITTI x 8: GuidanceHeads -> Affinity_Propagate(24, 3) with a sparse mask -> Wighted_L1_Loss -> backward() on a 16-bit x,
against the same step through x.float() and the float32 heads.
Each configuration runs in a child process of its own under a time limit; the first failure ends the run.
    python tools/bench_head_g16.py [--reps 80] [--B 8 64] [--dtype float16 bfloat16] [--step] [--json out.jsonl] [--only-engine] [--step-timeout 240]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK16, HBM = 2.5e15, 8e12
C, h, w = 64, 152, 608


def timed(fns, reps, blocks=5):
    """-> per function (median, min, max) ms of `blocks` event-timed blocks of `reps` calls; the functions' blocks alternate"""
    import torch
    for fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) / reps)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def put(row, name, t):
    row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = (round(v, 4) for v in t)


def compare(row, k):
    e, r = "engine_" + k, "f32route_" + k
    row[k + "_speedup"] = round(row[r + "_ms"] / row[e + "_ms"], 2)
    spreads = (row[e + "_max_ms"] - row[e + "_min_ms"]) + (row[r + "_max_ms"] - row[r + "_min_ms"])
    row[k + "_beats_bar"] = bool(row[r + "_ms"] - row[e + "_ms"] > spreads)


def child(B, dtn, reps, only_engine):
    import torch
    import cspn_amd  # noqa: F401
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    dt, f32 = getattr(torch, dtn), torch.float32
    H, W = 2 * h, 2 * w
    reps = max(1, reps * 8 // B)
    gen = torch.Generator(device="cuda").manual_seed(300 + B)
    x = torch.randn(B, C, h, w, device="cuda", generator=gen).to(dt)
    wg = torch.randn(8, C, 3, 3, device="cuda", generator=gen) / 24
    wb = torch.randn(1, C, 3, 3, device="cuda", generator=gen) / 24
    gg = torch.randn(B, 8, H, W, device="cuda", generator=gen)
    gb = torch.randn(B, 1, H, W, device="cuda", generator=gen)
    flop = 2.0 * 9 * C * 9 * B * h * w
    fwd_bytes = 2.0 * B * C * h * w + 36.0 * B * H * W
    bwd_bytes = 54.0 * B * H * W + 2 * (18.0 * B * H * W + 2.0 * B * C * h * w) + 2.0 * B * C * h * w
    row = dict(shape="kitti_x%d" % B, B=B, C=C, h=h, w=w, dtype=dtn, reps=reps)
    state = {}

    def eng_fwd():
        state["out"] = guidance_heads(x, wg, wb, guidance_dtype=f32)

    def eng_train():
        state["out"] = guidance_heads(x, wg, wb, guidance_dtype=f32)
        state["grads"] = guidance_heads_backward(x, wg, wb, gg, gb, guidance_dtype=f32)

    def rt_fwd():
        xf = x.float()
        state["rt_x"], state["rt_out"] = xf, guidance_heads(xf, wg, wb)

    def rt_train():
        rt_fwd()
        dx, dwg, dwb = guidance_heads_backward(state["rt_x"], wg, wb, gg, gb)
        state["rt_grads"] = (dx.to(dt), dwg, dwb)
    if only_engine:
        t = timed([eng_fwd, eng_train], reps)
        put(row, "engine_fwd", t[0])
        put(row, "engine_fwd_bw", t[1])
    else:
        t = timed([eng_fwd, rt_fwd, eng_train, rt_train], reps)
        for name, v in zip(("engine_fwd", "f32route_fwd", "engine_fwd_bw", "f32route_fwd_bw"), t):
            put(row, name, v)
    row["engine_fwd_bytes_frac"] = round(fwd_bytes / (row["engine_fwd_ms"] * 1e-3) / HBM, 3)
    row["engine_fwd_bw_bytes_frac"] = round((fwd_bytes + bwd_bytes) / (row["engine_fwd_bw_ms"] * 1e-3) / HBM, 3)
    row["engine_fwd_flop_frac"] = round(flop / (row["engine_fwd_ms"] * 1e-3) / PEAK16, 4)
    row["engine_fwd_bw_flop_frac"] = round(3 * flop / (row["engine_fwd_bw_ms"] * 1e-3) / PEAK16, 4)
    if not only_engine:
        def rel(a, b):
            return float((a.float() - b.float()).abs().max() / b.float().abs().max())
        compare(row, "fwd")
        compare(row, "fwd_bw")
        # (the route keeps the float32 weights and gradients unrounded: the difference is the rounding of the operands to dt, not an error of either)
        row.update(rel_diff_guidance=rel(state["out"][0], state["rt_out"][0]), rel_diff_blur=rel(state["out"][1], state["rt_out"][1]),
                   rel_diff_dx=rel(state["grads"][0], state["rt_grads"][0]), rel_diff_dwg=rel(state["grads"][1], state["rt_grads"][1]))
    print(json.dumps(row), flush=True)


def step_child(B, dtn, reps):
    """heads + 24 ring iterations + loss + backward, 16-bit x: GuidanceHeads against x.float() + the float32 heads"""
    import torch
    import cspn_amd
    from cspn_amd.train_utils import Wighted_L1_Loss, guidance_heads
    dt = getattr(torch, dtn)
    H, W = 2 * h, 2 * w
    gen = torch.Generator(device="cuda").manual_seed(400 + B)
    x = torch.randn(B, C, h, w, device="cuda", generator=gen).to(dt).requires_grad_(True)
    sp = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 0.05).float() * 2.0
    label = torch.rand(B, 1, H, W, device="cuda", generator=gen) * 3 + 0.5
    torch.manual_seed(1)
    heads = cspn_amd.GuidanceHeads(C, 3).cuda()
    prop, loss_fn = cspn_amd.Affinity_Propagate(24, 3), Wighted_L1_Loss()
    state = {}

    def finish(g, b, key):
        loss = loss_fn(prop(g, b, sp), label)
        loss.backward()
        state[key] = loss.detach()
        x.grad = heads.weight_guidance.grad = heads.weight_blur.grad = None

    def eng():
        finish(*heads(x), "engine_loss")

    def route():
        finish(*guidance_heads(x.float(), heads.weight_guidance, heads.weight_blur), "f32route_loss")
    row = dict(shape="kitti_x%d" % B, B=B, dtype=dtn, what="heads + Affinity_Propagate(24, 3) + Wighted_L1_Loss + backward", reps=reps)
    t = timed([eng, route], reps)
    put(row, "engine_step", t[0])
    put(row, "f32route_step", t[1])
    compare(row, "step")
    row.update({k: float(v) for k, v in state.items()})
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=80, help="calls per timed block at KITTI x 8 (scaled down with B)")
    ap.add_argument("--B", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--dtype", nargs="+", default=["float16", "bfloat16"], choices=["float16", "bfloat16"])
    ap.add_argument("--step", action="store_true", help="also the train step at KITTI x 8")
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-engine", action="store_true", help="the engine's calls only (profiling runs)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "step":
            step_child(int(a.child[1]), a.child[2], a.reps)
        else:
            child(int(a.child[1]), a.child[2], a.reps, a.only_engine)
        return 0
    rows = []
    jobs = [("heads", B, dtn) for B in a.B for dtn in a.dtype] + ([("step", 8, dtn) for dtn in a.dtype] if a.step else [])
    for what, B, dtn in jobs:
        cmd = ([sys.executable, os.path.abspath(__file__), "--child", what, str(B), dtn, "--reps", str(a.reps)] + (["--only-engine"] if a.only_engine else []))
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print("%s B %d %s: no result within %d s -- stopping" % (what, B, dtn, a.step_timeout), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("%s B %d %s: exit status %d -- stopping" % (what, B, dtn, r.returncode), file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        rows.append(line)
        print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            f.write("\n".join(rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
