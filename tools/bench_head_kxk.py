"""The guidance heads for 5x5 / 7x7 propagation (train_utils.guidance_heads with weight_guidance [24 | 48, C, 3, 3]: cspn_guidance_head_kxk_f32 and its
backward, three fp32 GEMMs on the matrix cores) against what a user had before them, on the same GPU in the same session:
  * slices   the composition of the 8-plane head: 3 (K = 5) or 6 (K = 7) calls of guidance_heads / guidance_heads_backward on weight slices of 8 (the blur head
             rides with the first), the outputs concatenated and the dL/dx parts summed in torch;
  * torch    the float32 op sequence of the reference layer: conv_transpose2d Unpool + conv2d (under autograd for forward + backward).
Shapes KITTI x 8 and KITTI x 64 (x [B,64,152,608] -> [B,K*K-1,304,1216] + [B,1,304,1216]), forward alone and forward + backward (all three gradients).
Every time is the median of 5 prewarmed blocks of event-timed calls (torch: 3 blocks of one call); min and max of the blocks are kept as the spread.
    useful_frac   2 * 9 * C * O * B * h * w FLOP (O = K*K planes incl. blur) / time / 157.3 TFLOP/s (the fp32 peak of vector unit and matrix cores alike)
    padded_frac   O / (O rounded up to the matrix block: 32 or 64): the share of the issued matrix FLOP that is useful
Each (K, B) configuration runs in a child process of its own under a time limit; the first failure ends the run.
    python tools/bench_head_kxk.py [--reps 5] [--K 5 7] [--B 8 64] [--json out.jsonl] [--only-engine] [--step-timeout 240]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 157.3e12
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


def child(K, B, reps, only_engine):
    import torch
    import torch.nn.functional as TF
    import cspn_amd  # noqa: F401
    from cspn_amd.train_utils import guidance_heads, guidance_heads_backward
    P, O = K * K - 1, K * K
    H, W = 2 * h, 2 * w
    gen = torch.Generator(device="cuda").manual_seed(K * 100 + B)
    x = torch.randn(B, C, h, w, device="cuda", generator=gen)
    wg = torch.randn(P, C, 3, 3, device="cuda", generator=gen) / 24
    wb = torch.randn(1, C, 3, 3, device="cuda", generator=gen) / 24
    gg = torch.randn(B, P, H, W, device="cuda", generator=gen)
    gb = torch.randn(B, 1, H, W, device="cuda", generator=gen)
    flop = 2.0 * 9 * C * O * B * h * w
    row = dict(shape="kitti_x%d" % B, B=B, C=C, h=h, w=w, K=K, planes=O, padded_frac=round(O / ((O + 31) // 32 * 32), 3))

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
    row["engine_fwd_useful_frac"] = round(flop / (row["engine_fwd_ms"] * 1e-3) / PEAK, 3)
    row["engine_fwd_bw_useful_frac"] = round(3 * flop / (row["engine_fwd_bw_ms"] * 1e-3) / PEAK, 3)
    if not only_engine:
        slices = [wg[s:s + 8].contiguous() for s in range(0, P, 8)]
        gslices = [gg[:, s:s + 8].contiguous() for s in range(0, P, 8)]     # (cut once, outside the timed region)

        def sl_fwd():
            parts = [guidance_heads(x, ws_, wb if i == 0 else None) for i, ws_ in enumerate(slices)]
            state["sl_out"] = (torch.cat([p[0] for p in parts], 1), parts[0][1])

        def sl_train():
            sl_fwd()
            dx, dws, dwb = None, [], None
            for i, ws_ in enumerate(slices):
                pdx, pdw, pdb = guidance_heads_backward(x, ws_, wb if i == 0 else None, gslices[i], gb if i == 0 else None)
                dx = pdx if dx is None else dx.add_(pdx)
                dws.append(pdw)
                dwb = pdb if i == 0 else dwb
            state["sl_grads"] = (dx, torch.cat(dws, 0), dwb)
        put("slices_fwd", timed(sl_fwd, reps))
        put("slices_fwd_bw", timed(sl_train, reps))
        up = torch.zeros(C, 1, 2, 2, device="cuda")
        up[:, :, 0, 0] = 1
        wall = torch.cat([wg, wb], 0)

        def th_fwd():
            with torch.no_grad():
                state["th_out"] = TF.conv2d(TF.conv_transpose2d(x, up, stride=2, groups=C), wall, padding=1)
        xt, wt = x.clone().requires_grad_(True), wall.clone().requires_grad_(True)
        gall = torch.cat([gg, gb], 1)

        def th_train():
            xt.grad = wt.grad = None
            TF.conv2d(TF.conv_transpose2d(xt, up, stride=2, groups=C), wt, padding=1).backward(gall)
        put("torch_fwd", timed(th_fwd, 1, blocks=3))
        put("torch_fwd_bw", timed(th_train, 1, blocks=3))

        def rel(a, b):
            return float((a - b).abs().max() / b.abs().max())
        g, b = state["out"]
        dx, dwg, dwb = state["grads"]
        row.update(fwd_speedup_vs_slices=round(row["slices_fwd_ms"] / row["engine_fwd_ms"], 2),
                   fwd_bw_speedup_vs_slices=round(row["slices_fwd_bw_ms"] / row["engine_fwd_bw_ms"], 2),
                   fwd_speedup_vs_torch=round(row["torch_fwd_ms"] / row["engine_fwd_ms"], 2),
                   fwd_bw_speedup_vs_torch=round(row["torch_fwd_bw_ms"] / row["engine_fwd_bw_ms"], 2),
                   rel_err_guidance_vs_slices=rel(g, state["sl_out"][0]), rel_err_dx_vs_slices=rel(dx, state["sl_grads"][0]),
                   rel_err_dwg_vs_slices=rel(dwg, state["sl_grads"][1]), rel_err_guidance_vs_torch=rel(g, state["th_out"][:, :P]),
                   rel_err_dx_vs_torch=rel(dx, xt.grad), rel_err_dwg_vs_torch=rel(dwg, wt.grad[:P]))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[5, 7])
    ap.add_argument("--B", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--json", default=None)
    ap.add_argument("--only-engine", action="store_true", help="the engine's calls only (profiling runs)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per (K, B) child process")
    ap.add_argument("--child", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.reps, a.only_engine)
        return 0
    rows = []
    for K in a.K:
        for B in a.B:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(K), str(B), "--reps", str(a.reps)] + (["--only-engine"] if a.only_engine else [])
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print("K %d B %d: no result within %d s -- stopping" % (K, B, a.step_timeout), file=sys.stderr)
                return 124
            if r.returncode != 0:
                print("K %d B %d: exit status %d -- stopping" % (K, B, r.returncode), file=sys.stderr)
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
