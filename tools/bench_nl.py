"""Non-local propagation with learned offsets (cspn2d_forward_nl / cspn2d_backward_nl) beside the float32 torch statement of the same contract on
the same GPU: the grid_sample loop a port writes today (one grid per neighbour, built once per call; n_iter x 8 grid_sample calls; autograd keeps
every level and every sampling for the training case).  Writes profiles/nl.md, the only source of the figures DESIGN.md §3.4j quotes.
Shape KITTI x 8 (B 8, 1 x 304 x 1216), n_iter 18, C 1, affinities randn * 0.2, ~500 measured points per image.  Offsets: `random` (randn * 1.5,
independent per pixel) and `smooth` (a 15 x 15 box low-pass of the same draw, rescaled to the same standard deviation: what a trained offset head
looks like to the memory system).  Measured: the forward alone, a training step (the forward that keeps its history, then the backward for all
three gradients), the backward alone, and peak memory.  The engine and the statement take turns block by block; every time is the median of the
prewarmed blocks of event-timed calls, min / max over the blocks are the spread within the run.  Next to the times: the forward's algorithmic
bytes (4 * 3 KK + 8 C per pixel and step) over its time against the 8 TB/s roofline, and the bytes the adjoint adds with float atomics over
the backward's time against the chip-wide float-atomic rate of ~1.3 TB/s: (4 KK + 1) * 4 C per pixel and step are added in all (in LDS, when
every corner is inside), of which at most 4 C * (76 * 28) / (64 * 16) reach global memory as atomics (the window of a 64 x 16 tile).  No ratio is fixed in advance; the one condition is that the engine's forward and
training step are each faster than the statement in the same run, and the file says so either way.
    python tools/bench_nl.py [--reps 3] [--blocks 3] [--md profiles/nl.md] [--json out.jsonl] [--no-torch]"""
import argparse
import json
import os
import sys

import torch

KK, N_ITER, C = 8, 18, 1
B, H, W = 8, 304, 1216
BASES = [(t - 1, l - 1) for t in range(3) for l in range(3) if (t, l) != (1, 1)]

# what the compiler reports for cspn_amd/csrc/cspn2d_nl.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, --save-temps
# for the disassembly): not measured by this tool, recorded here so that the profile has one source
BUILD_REPORT = """\
| kernel | VGPRs | AGPRs | scratch | occupancy (waves / SIMD) |
|---|---|---|---|---|
| `nl_forward_step<3, VEC>` (four pixels a thread, 16-byte loads) | 242 | 0 | 0 | 2 |
| `nl_forward_step<3, scalar>` (guarded scalar loads: odd widths, misaligned views) | 256 | 86 | 0 | 1 |
| `nl_adjoint_step<3>` (one pixel a lane, four rows in turn; an LDS window of 8,512 bytes) | 52 | 0 | 0 | 8 |
| `nl_gate_grad<3>` (one pixel a lane, `__launch_bounds__(256, 4)`) | 128 | 0 | 0 | 4 |
| `nl_pin` (four instances) | 8 - 12 | 0 | 0 | 8 |
| `nl_sample_kernel<3>` | 49 | 0 | 0 | 8 |
| `nl_sample_backward_kernel<3>` | 32 | 0 | 0 | 8 |

No kernel uses scratch.  The scalar forward instance keeps its 86 overflow registers in AGPRs (one wave per SIMD): it serves odd widths and
misaligned views only.  Before the corner indices were kept out of the loop-invariant set (the `asm volatile("" : "+v"(i00))` in the channel
loop) the compiler held all 128 corner addresses of a thread across the channel loop: 256 VGPRs + 172 AGPRs in the vector instance, and 304
bytes of scratch in the gate gradient under its occupancy bound.

The float atomics, read once in the unit's disassembly: 67 `global_atomic_add_f32 v[..], v.., off` and 33 `ds_add_f32` (neither returns a
value), 0 occurrences of `cmpswap` / `cmpst`: each `atomicAdd(float*)`, on global memory and on LDS, is one hardware float add, no
compare-and-swap loop.

The adjoint step first scattered straight from the lanes: 4 KK + 1 = 33 global float atomics a pixel and step, each wave instruction's 64 adds
wherever the 64 offsets pointed.  Measured once at this shape before the LDS window was added (18 sweeps, `grad_x` only, ms): 53.9 with the
`random` offsets, 44.2 with `smooth`, 30.0 with a 63 x 63 low-pass, 8.8 with one constant offset for all pixels (adjacent addresses: 0.8 TB/s of
added bytes) and 2.1 with zero offsets (24 of the 33 weights vanish).  The access shape, not the byte count, set the time: adjacent pixels'
offsets differ by half a pixel even in the `smooth` field, so a wave instruction's adds fell into several rows in pieces of a few bytes.  With
the window the same sweeps take 9.5 / 9.7 / 9.7 / 9.4 / 2.8 ms: the time no longer depends on how smooth the offsets are."""


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


def torch_nl(aff, off, x, sparse, n):
    """the float32 statement: grid_sample(align_corners=True, padding_mode='zeros') at p + base_k + offset_k(p), the grids built once per call"""
    Bn, Cn, Hn, Wn = x.shape
    ys = torch.arange(Hn, device=x.device, dtype=x.dtype).view(1, Hn, 1)
    xs = torch.arange(Wn, device=x.device, dtype=x.dtype).view(1, 1, Wn)
    grids = [torch.stack((2 * (xs + bx + off[:, 2 * k + 1]) / (Wn - 1) - 1, 2 * (ys + by + off[:, 2 * k]) / (Hn - 1) - 1), -1) for k, (by, bx) in enumerate(BASES)]
    m = (sparse > 0).to(x.dtype)
    c = 1 - aff.sum(1, keepdim=True)
    h = x
    for _ in range(n):
        ht = (1 - m) * h + m * sparse
        h = c * ht + sum(aff[:, k:k + 1] * torch.nn.functional.grid_sample(ht, grids[k], mode="bilinear", padding_mode="zeros", align_corners=True)
                         for k in range(len(BASES)))
    return h


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def fmt(s):
    return "%.3f (%.3f - %.3f)" % (s["ms"], s["min"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nl.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-torch", action="store_true", help="the engine calls only (no comparison: the profile is not written)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cspn_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_nl.py measures on the GPU; none found")
    gen = torch.Generator(device="cuda").manual_seed(18)
    aff = torch.randn(B, KK, H, W, device="cuda", generator=gen) * 0.2
    draw = torch.randn(B, 2 * KK, H, W, device="cuda", generator=gen) * 1.5
    low = torch.nn.functional.avg_pool2d(draw, 15, 1, 7)
    fields = {"random": draw, "smooth": low * (draw.std() / low.std())}
    x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
    s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 500 / (H * W)).float() * (x[:, :1] * 0.5 + 0.1)
    go = torch.randn(B, C, H, W, device="cuda", generator=gen)
    px = B * H * W
    rows = []
    for name, off in fields.items():
        off = off.contiguous()
        row = dict(shape="kitti_x8", B=B, C=C, H=H, W=W, n_iter=N_ITER, offsets=name, offset_std=round(float(off.std()), 3))
        state = {}

        def eng_fwd():
            return F.cspn2d_forward_nl(aff, off, x, s, N_ITER)

        def eng_train():
            out, hist = F.cspn2d_forward_nl(aff, off, x, s, N_ITER, return_history=True)
            state["hist"] = hist
            state["grads"] = F.cspn2d_backward_nl(aff, off, x, s, go, N_ITER, history=hist)

        def eng_bwd():
            F.cspn2d_backward_nl(aff, off, x, s, go, N_ITER, history=state["hist"])
        leaves = [t.clone().requires_grad_(True) for t in (aff, off, x)]

        def torch_fwd():
            with torch.no_grad():
                return torch_nl(aff, off, x, s, N_ITER)

        def torch_train():
            for t in leaves:
                t.grad = None
            torch_nl(*leaves, s, N_ITER).backward(go)
        fns_f, fns_t = {"engine": eng_fwd}, {"engine": eng_train}
        if not a.no_torch:
            fns_f["torch"], fns_t["torch"] = torch_fwd, torch_train
        tf = blocks_of(fns_f, a.reps, a.blocks)
        tt = blocks_of(fns_t, a.reps, a.blocks)
        tb = blocks_of({"engine": eng_bwd}, a.reps, a.blocks)
        row.update(engine_fwd=stats(tf["engine"]), engine_train=stats(tt["engine"]), engine_bwd=stats(tb["engine"]),
                   engine_fwd_mib=peak_mib(eng_fwd), engine_train_mib=peak_mib(eng_train))
        fwd_bytes = (4 * 3 * KK + 8 * C) * px * N_ITER
        atomic_bytes = (4 * KK + 1) * 4 * C * px * N_ITER                      # added in all, nearly all of it in LDS
        global_atomic_bytes = 4 * C * (76 * 28) / (64 * 16) * px * N_ITER      # the windows' adds to global memory (an upper bound: empty cells are skipped)
        row.update(fwd_algorithmic_gb=round(fwd_bytes / 1e9, 3), fwd_tb_per_s=round(fwd_bytes / (row["engine_fwd"]["ms"] * 1e-3) / 1e12, 3),
                   fwd_share_of_8tb_roofline=round(fwd_bytes / (row["engine_fwd"]["ms"] * 1e-3) / 8e12, 3),
                   adjoint_atomic_gb=round(atomic_bytes / 1e9, 3), atomic_tb_per_s_over_bwd=round(atomic_bytes / (row["engine_bwd"]["ms"] * 1e-3) / 1e12, 3),
                   global_atomic_gb=round(global_atomic_bytes / 1e9, 3), global_atomic_floor_ms=round(global_atomic_bytes / 1.3e12 * 1e3, 3),
                   atomic_floor_ms=round(atomic_bytes / 1.3e12 * 1e3, 3))
        if not a.no_torch:
            row.update(torch_fwd=stats(tf["torch"]), torch_train=stats(tt["torch"]), torch_fwd_mib=peak_mib(torch_fwd), torch_train_mib=peak_mib(torch_train),
                       torch_over_engine_fwd=round(tf["torch"][len(tf["torch"]) // 2] / row["engine_fwd"]["ms"], 2),
                       torch_over_engine_train=round(tt["torch"][len(tt["torch"]) // 2] / row["engine_train"]["ms"], 2))
            torch_train()
            eng_train()
            row.update(rel_err_out=rel(eng_fwd(), torch_fwd()),
                       **{"rel_err_" + k: rel(g, l.grad) for k, g, l in zip(("daff", "doffset", "dx"), state["grads"], leaves)})
        del leaves
        state.clear()
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if a.no_torch:
        return
    faster = all(r["engine_fwd"]["ms"] < r["torch_fwd"]["ms"] and r["engine_train"]["ms"] < r["torch_train"]["ms"] for r in rows)
    L = ["# Non-local propagation with learned offsets: `cspn2d_forward_nl` / `cspn2d_backward_nl`", "",
         "Written by `tools/bench_nl.py` (reps %d, blocks %d) on %s, torch %s.  Shape KITTI x 8: B %d, C %d, %d x %d, n_iter %d, K 3; affinities randn * 0.2, "
         "~500 measured points per image.  Times in ms: median (min - max) over the blocks of one run, the engine and the torch statement taking turns."
         % (a.reps, a.blocks, torch.cuda.get_device_name(0), torch.__version__, B, C, H, W, N_ITER), "",
         "The torch statement is the float32 `grid_sample` loop of the same contract (grids built once per call, %d `grid_sample` calls a forward), under "
         "autograd for the training step." % (N_ITER * KK), "",
         "## Times and peak memory", "",
         "| offsets | engine forward | torch forward | torch / engine | engine training step | torch training step | torch / engine | engine backward alone |",
         "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %s (std %.2f) | %s | %s | %.2f | %s | %s | %.2f | %s |" % (r["offsets"], r["offset_std"], fmt(r["engine_fwd"]), fmt(r["torch_fwd"]), r["torch_over_engine_fwd"],
                                                                          fmt(r["engine_train"]), fmt(r["torch_train"]), r["torch_over_engine_train"], fmt(r["engine_bwd"])))
    L += ["", "| offsets | engine forward MiB | torch forward MiB | engine training step MiB | torch training step MiB |", "|---|---|---|---|---|"]
    for r in rows:
        L.append("| %s | %.1f | %.1f | %.1f | %.1f |" % (r["offsets"], r["engine_fwd_mib"], r["torch_fwd_mib"], r["engine_train_mib"], r["torch_train_mib"]))
    L += ["", "**The condition** (the engine's forward and its training step each faster than the torch statement measured in the same run): %s."
          % ("holds for both offset fields" if faster else "DOES NOT HOLD -- see the rows above"), "",
          "## Against the hardware's rates", "",
          "Forward: the algorithmic bytes are 4 * 3 KK + 8 C = %d per pixel and step (the 24 affinity / offset planes once, the level read and written once; the 32 "
          "gathered corners are counted as cache hits).  Adjoint: the scatter adds (4 KK + 1) * 4 C = %d bytes per pixel and step when every corner is inside and no "
          "weight is zero.  They are summed in an LDS window per 64 x 16 tile; what reaches global memory as float atomics is the window, at most 4 C * 76 * 28 / 1024 "
          "= %.1f bytes per pixel and step.  The chip-wide float-atomic rate is ~1.3 TB/s of added bytes: the floor columns are the time those bytes alone take at that "
          "rate (all added bytes, had they gone to global memory; and the windows' bytes, which do).  The backward's time also holds the memsets, the gate and offset "
          "gradient pass and the pre-pass; the adjoint is bound by the LDS adds, not by the global atomic rate." % (4 * 3 * KK + 8 * C, (4 * KK + 1) * 4 * C, 4 * C * 76 * 28 / 1024), "",
          "| offsets | forward bytes (GB) | forward TB/s | share of the 8 TB/s roofline | added bytes (GB) | added TB/s over the whole backward | floor at 1.3 TB/s (ms) | "
          "global atomic bytes (GB) | their floor (ms) |",
          "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        L.append("| %s | %.3f | %.3f | %.1f %% | %.3f | %.3f | %.3f | %.3f | %.3f |" % (
            r["offsets"], r["fwd_algorithmic_gb"], r["fwd_tb_per_s"], 100 * r["fwd_share_of_8tb_roofline"], r["adjoint_atomic_gb"], r["atomic_tb_per_s_over_bwd"],
            r["atomic_floor_ms"], r["global_atomic_gb"], r["global_atomic_floor_ms"]))
    L += ["", "## Results at the timed size", "",
          "max |engine - torch| / max |torch|, both float32 (the statement samples at the absolute coordinate, the engine takes the fraction from the offset; "
          "the float64 comparisons are in `tests/test_nl.py`, where every gradient of the engine is within 1e-6 of the statement; the larger grad_offset figure here is the float32 statement's own: its fraction comes from a normalised absolute coordinate of up to 1216, so its bilinear weights carry ~1e-4 of error):", "",
          "| offsets | out | grad_aff | grad_offset | grad_x |", "|---|---|---|---|---|"]
    for r in rows:
        L.append("| %s | %.2e | %.2e | %.2e | %.2e |" % (r["offsets"], r["rel_err_out"], r["rel_err_daff"], r["rel_err_doffset"], r["rel_err_dx"]))
    L += ["", "## What the compiler made (not measured by this tool: read from the build)", "", BUILD_REPORT, ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("\n".join(L))


if __name__ == "__main__":
    main()
