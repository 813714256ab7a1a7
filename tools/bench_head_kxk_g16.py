"""The guidance heads for 5x5 / 7x7 propagation on a float16 / bfloat16 feature map (train_utils.guidance_heads with a 16-bit x and weight_guidance
[24 | 48, C, 3, 3]: cspn_guidance_head_kxk_g16 and its backward, three GEMMs on the 16-bit matrix instructions) against the route a user had before them, on
the same GPU in the same session:
  * f32route   the float32 entry points on x.float() plus .to(dt) of the guidance (forward), and on .float() of dL/dguidance plus .to(dt) of dL/dx (backward;
               the forward's x.float() is kept, as an autograd Function would keep it).
Shapes KITTI x 8 and KITTI x 64 (x [B,64,152,608] -> [B,K*K-1,304,1216] + [B,1,304,1216]), both dtypes, forward alone and forward + backward (all three
gradients).  Every time is the median of 5 prewarmed blocks of event-timed calls; min and max of the blocks are kept as the spread.
    *_bytes_frac   the call's own bytes (x 2 B per input pixel and channel, guidance 2 (K*K-1) B and blur 4 B per output pixel; backward: the same tensors read
                   twice -- dL/dx and dL/dW -- plus dL/dx written) / time / 8 TB/s
    *_flop_frac    2 * 9 * C * O * B * h * w FLOP (O = K*K planes incl. blur; three such GEMMs with the backward) / time / 2.5 PFLOP/s (the 16-bit matrix peak)
    beats_bar      the 16-bit call is faster than the route by more than the two spreads together
Each (K, B, dtype) configuration runs in a child process of its own under a time limit; the first failure ends the run.
    python tools/bench_head_kxk_g16.py [--reps 5] [--K 5 7] [--B 8 64] [--dtype float16 bfloat16] [--json out.jsonl] [--only-engine] [--step-timeout 240]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK16, HBM = 2.5e15, 8e12
C, h, w = 64, 152, 608


def timed(fn, reps, blocks=5):
    import torch
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
    return ts[len(ts) // 2], ts[0], ts[-1]


def child(K, B, dtn, reps, only_engine):
    import torch
    import cspn_amd  # noqa: F401
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    dt = getattr(torch, dtn)
    P, O = K * K - 1, K * K
    H, W = 2 * h, 2 * w
    gen = torch.Generator(device="cuda").manual_seed(K * 100 + B)
    x = torch.randn(B, C, h, w, device="cuda", generator=gen).to(dt)
    wg = torch.randn(P, C, 3, 3, device="cuda", generator=gen) / 24
    wb = torch.randn(1, C, 3, 3, device="cuda", generator=gen) / 24
    gg = torch.randn(B, P, H, W, device="cuda", generator=gen).to(dt)
    gb = torch.randn(B, 1, H, W, device="cuda", generator=gen)
    flop = 2.0 * 9 * C * O * B * h * w
    fwd_bytes = 2.0 * B * C * h * w + (2.0 * P + 4) * B * H * W
    bwd_bytes = 2 * fwd_bytes + 2.0 * B * C * h * w
    row = dict(shape="kitti_x%d" % B, B=B, C=C, h=h, w=w, K=K, dtype=dtn, planes=O)

    def put(name, t):
        row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = (round(v, 3) for v in t)

    state = {}

    def eng_fwd():
        state["out"] = guidance_heads(x, wg, wb)

    def eng_train():
        state["out"] = guidance_heads(x, wg, wb)
        state["grads"] = guidance_heads_backward(x, wg, wb, gg, gb)
    put("engine_fwd", timed(eng_fwd, reps))
    put("engine_fwd_bw", timed(eng_train, reps))
    row["engine_fwd_bytes_frac"] = round(fwd_bytes / (row["engine_fwd_ms"] * 1e-3) / HBM, 3)
    row["engine_fwd_bw_bytes_frac"] = round((fwd_bytes + bwd_bytes) / (row["engine_fwd_bw_ms"] * 1e-3) / HBM, 3)
    row["engine_fwd_flop_frac"] = round(flop / (row["engine_fwd_ms"] * 1e-3) / PEAK16, 4)
    row["engine_fwd_bw_flop_frac"] = round(3 * flop / (row["engine_fwd_bw_ms"] * 1e-3) / PEAK16, 4)
    if not only_engine:
        def rt_fwd():
            xf = x.float()
            g, b = guidance_heads(xf, wg, wb)
            state["rt_x"], state["rt_out"] = xf, (g.to(dt), b)

        def rt_train():
            rt_fwd()
            dx, dwg, dwb = guidance_heads_backward(state["rt_x"], wg, wb, gg.float(), gb)
            state["rt_grads"] = (dx.to(dt), dwg, dwb)
        put("f32route_fwd", timed(rt_fwd, reps))
        put("f32route_fwd_bw", timed(rt_train, reps))

        def rel(a, b):
            return float((a.float() - b.float()).abs().max() / b.float().abs().max())
        for k in ("fwd", "fwd_bw"):
            e, r = "engine_" + k, "f32route_" + k
            row[k + "_speedup"] = round(row[r + "_ms"] / row[e + "_ms"], 2)
            spreads = (row[e + "_max_ms"] - row[e + "_min_ms"]) + (row[r + "_max_ms"] - row[r + "_min_ms"])
            row[k + "_beats_bar"] = bool(row[r + "_ms"] - row[e + "_ms"] > spreads)
        row.update(rel_diff_guidance=rel(state["out"][0], state["rt_out"][0]), rel_diff_blur=rel(state["out"][1], state["rt_out"][1]),
                   rel_diff_dx=rel(state["grads"][0], state["rt_grads"][0]), rel_diff_dwg=rel(state["grads"][1], state["rt_grads"][1]))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--B", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--dtype", nargs="+", default=["float16", "bfloat16"], choices=["float16", "bfloat16"])
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-engine", action="store_true", help="the engine's calls only (profiling runs)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per (K, B, dtype) child process")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.child[2], a.reps, a.only_engine)
        return 0
    rows = []
    for K in a.K:
        for B in a.B:
            for dtn in a.dtype:
                cmd = ([sys.executable, os.path.abspath(__file__), "--child", str(K), str(B), dtn, "--reps", str(a.reps)]
                       + (["--only-engine"] if a.only_engine else []))
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.step_timeout)
                except subprocess.TimeoutExpired:
                    print("K %d B %d %s: no result within %d s -- stopping" % (K, B, dtn, a.step_timeout), file=sys.stderr)
                    return 124
                if r.returncode != 0:
                    print("K %d B %d %s: exit status %d -- stopping" % (K, B, dtn, r.returncode), file=sys.stderr)
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
