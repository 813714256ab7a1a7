"""K x K propagation with per-step attention (cspn_amd.Dynamic_Propagate: cspn2d_forward_kxk_dyn / cspn2d_backward_kxk_dyn) against the route it
replaces, in the same process on the same GPU:
    composed   per step, in torch under autograd: the gates modulated by the step's attention (a gather of the ring planes times the guidance),
               D, the division, the centre term, the pin; one one-step cspn2d_forward_kxk call (the engine's autograd Function) on the
               normalised gates.  n float32 tensors [B,KK,H,W] are written, read back and kept for the backward, n normalisation backwards follow
    dyn        the module: one forward call, one backward call, no gate-sized tensor besides the guidance and the attention
KITTI x 8 (B 8, 304 x 1216), n = 6, K 5 and 7, C = 1, float32, about 5 % of the pixels measured.  The two routes alternate within a round and the
rounds repeat; a time is the median over the rounds of the per-round median of --reps prewarmed event-timed blocks, "spread" is (max - min) /
median over the rounds.  Peak memory is max_memory_allocated over one call less what was allocated before it.  The forward's roofline fraction
uses the dyn route's algorithmic bytes, n (4 KK + 4 (R+1) + 8 C + 4) per pixel, over 8 TB/s.
    python tools/bench_kxk_dyn.py [--reps 3] [--rounds 3] [--shape B H W] [--K 5 7] [--resources remarks.txt] [--out profiles/kxk_dyn.md]
--resources: the compiler's -Rpass-analysis=kernel-resource-usage remarks of cspn2d_kxk_dyn.hip, for the profile's resource table."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cspn_amd  # noqa: E402
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


def composed(g, att, x, s, K, n):
    """the contract with torch modulation and normalisation around n one-step engine calls"""
    R = K // 2
    rings = torch.tensor([max(abs(R - t), abs(R - l)) for t in range(K) for l in range(K) if (t, l) != (R, R)], device=g.device)
    H = x
    for t in range(n):
        a = att[:, t * (R + 1):(t + 1) * (R + 1)]
        wh = a[:, rings] * g
        D = a[:, :1] + wh.abs().sum(1, keepdim=True)
        w = wh / D
        Ht = H if s is None else torch.where(s > 0, s, H)
        H = (1 - w.sum(1, keepdim=True)) * Ht + F._AffinityPropagateKxKFunction.apply(Ht, w, K, 1)
    return H


def resource_table(path):
    """the remarks file -> markdown rows: kernel instance, VGPRs, AGPRs, scratch, waves per SIMD, LDS bytes"""
    text = open(path).read()
    rows = []
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", text, re.S):
        name = m.group(1)
        k = re.search(r"(kxk_dyn_[a-z_]+?)I((?:L[ib]\d+E)+)E", name)   # the template arguments of the mangled name: (K, [PX,] VEC)
        if not k:
            continue
        targs = re.findall(r"L([ib])(\d+)E", k.group(2))
        ints = [v for kind, v in targs if kind == "i"]
        label = "%s<%s>" % (k.group(1), ", ".join(["%s=%s" % p for p in zip(("K", "PX"), ints)] + ["VEC" if targs[-1][1] == "1" else "scalar"]))
        row = "| `%s` | %s | %s | %s | %s | %s |" % ((label,) + m.groups()[1:])
        if row not in rows:
            rows.append(row)
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=3, default=(8, 304, 1216), metavar=("B", "H", "W"))
    ap.add_argument("--K", type=int, nargs="+", default=(5, 7))
    ap.add_argument("--n", type=int, default=6)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kxk_dyn.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    B, H, W = a.shape
    n, C = a.n, 1
    rows = []
    for K in a.K:
        KK, R = K * K - 1, K // 2
        gen = torch.Generator(device="cuda").manual_seed(K)
        g = (torch.rand(B, KK, H, W, device="cuda", generator=gen) + 0.05) * (torch.rand(B, KK, H, W, device="cuda", generator=gen) < 0.5).float().mul_(2).sub_(1)
        att = torch.rand(B, n * (R + 1), H, W, device="cuda", generator=gen) + 0.25
        x = torch.rand(B, C, H, W, device="cuda", generator=gen) * 10
        s = (torch.rand(B, 1, H, W, device="cuda", generator=gen) < 0.05).float() * (torch.rand(B, 1, H, W, device="cuda", generator=gen) * 10 + 0.1)
        go = torch.randn(B, C, H, W, device="cuda", generator=gen)
        m = cspn_amd.Dynamic_Propagate(n, K)
        leaves = [t.clone().requires_grad_(True) for t in (g, att, x)]

        def step(route):
            for t in leaves:
                t.grad = None
            out = route(*leaves)
            out.backward(go)
            return out

        def dyn_fwd():
            with torch.no_grad():
                return m(g, att, x, s)

        def composed_fwd():
            with torch.no_grad():
                return composed(g, att, x, s, K, n)

        variants = {"composed_fwd": composed_fwd, "dyn_fwd": dyn_fwd, "composed_step": lambda: step(lambda gg, aa, xx: composed(gg, aa, xx, s, K, n)),
                    "dyn_step": lambda: step(lambda gg, aa, xx: m(gg, aa, xx, s))}
        ts = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ts[k].append(timed(fn, a.reps))
        t = {k: med(v) for k, v in ts.items()}
        spread = {k: (max(v) - min(v)) / t[k] for k, v in ts.items()}
        mem = {k: peak_bytes(fn) for k, fn in variants.items()}
        ref, got = composed_fwd(), dyn_fwd()
        err = float((ref - got).abs().max() / ref.abs().max())
        step(lambda gg, aa, xx: composed(gg, aa, xx, s, K, n))
        ref_g = [t_.grad.clone() for t_ in leaves]
        step(lambda gg, aa, xx: m(gg, aa, xx, s))
        gerr = [float((r - t_.grad).abs().max() / r.abs().max()) for r, t_ in zip(ref_g, leaves)]
        bytes_fwd = B * H * W * n * (4 * KK + 4 * (R + 1) + 8 * C + 4)
        row = dict(B=B, C=C, H=H, W=W, K=K, n_iter=n, rounds=a.rounds, reps=a.reps, **{k + "_ms": round(v, 3) for k, v in t.items()},
                   **{k + "_spread": round(v, 4) for k, v in spread.items()}, **{k + "_peak_mb": round(v / 2 ** 20, 1) for k, v in mem.items()},
                   fwd_ratio=round(t["composed_fwd"] / t["dyn_fwd"], 3), step_ratio=round(t["composed_step"] / t["dyn_step"], 3),
                   dyn_fwd_roofline=round(bytes_fwd / (t["dyn_fwd"] * 1e-3) / PEAK, 3), fwd_max_rel_diff=err, grad_max_rel_diff=gerr)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del g, att, x, s, go, leaves, ref, got, ref_g
        torch.cuda.empty_cache()
    lines = ["# K x K propagation with per-step attention (`cspn2d_*_kxk_dyn_*`, DESIGN.md §3.4k)", "",
             "Written by `tools/bench_kxk_dyn.py`; the only source of figures for §3.4k.", ""]
    if a.resources:
        lines += ["## Resources of every kernel instance (gfx950, `-Rpass-analysis=kernel-resource-usage`)", "",
                  "| instance | VGPRs | AGPRs | scratch bytes / lane | waves / SIMD | LDS bytes / workgroup |", "|---|---|---|---|---|---|"]
        lines += resource_table(a.resources) + [""]
    lines += ["## Measured on one MI355X: %s, B %d, %d x %d, n = %d, C = 1, float32, with sparse (5 %% measured)" % (torch.cuda.get_device_name(0), B, H, W, n), "",
              "`composed`: torch modulation and normalisation around n one-step `cspn2d_forward_kxk` calls plus the centre term, under autograd; `dyn`: "
              "`Dynamic_Propagate`.  Median over %d rounds of the per-round median of 5 blocks of %d calls; spread = (max - min) / median over the rounds; "
              "peak = `max_memory_allocated` over one call less what was allocated before it.  A ratio above 1 means `dyn` is faster." % (a.rounds, a.reps), "",
              "| K | forward composed ms (spread) | forward dyn ms (spread) | ratio | dyn forward share of the 8 TB/s roofline | training step composed ms (spread) | "
              "training step dyn ms (spread) | ratio | peak forward composed / dyn MiB | peak training step composed / dyn MiB | max rel. difference out / dL/dguidance, "
              "dL/datt, dL/dx |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %d | %.3f (%.1f %%) | %.3f (%.1f %%) | %.2f | %.3f | %.3f (%.1f %%) | %.3f (%.1f %%) | %.2f | %.1f / %.1f | %.1f / %.1f | %.2g / %s |" % (
            r["K"], r["composed_fwd_ms"], 100 * r["composed_fwd_spread"], r["dyn_fwd_ms"], 100 * r["dyn_fwd_spread"], r["fwd_ratio"], r["dyn_fwd_roofline"],
            r["composed_step_ms"], 100 * r["composed_step_spread"], r["dyn_step_ms"], 100 * r["dyn_step_spread"], r["step_ratio"],
            r["composed_fwd_peak_mb"], r["dyn_fwd_peak_mb"], r["composed_step_peak_mb"], r["dyn_step_peak_mb"], r["fwd_max_rel_diff"],
            ", ".join("%.2g" % e for e in r["grad_max_rel_diff"])))
    lines += ["", "Raw rows:", "", "```"] + [json.dumps(r) for r in rows] + ["```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
