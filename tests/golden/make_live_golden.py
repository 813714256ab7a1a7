"""Generates tests/golden/live_reference_golden.npz and tests/golden/reference_digests.json: what the UNMODIFIED reference returns
for the inputs of the tests that compare against it directly (tests/test_oracle.py, test_head.py, test_backward.py), so that those
tests run without the reference tree.

* live_reference_golden.npz: the reference's outputs for the seeded inputs those tests generate (the inputs are not stored: the
  tests rebuild them from the same seeds).
* reference_digests.json: sha256 digests of the arrays the reference produces for the committed fixtures
  cspn2d_norm_golden.npz (affinity_normalization on the guidance of cspn2d_golden.npz) and aux_golden.npz (utils.py /
  loss.py through make_aux_golden.py), computed from the reference's own outputs, never from the fixtures.

Run in the authoring container only (needs the reference tree, oracle/ref_harness.py):
    python tests/golden/make_live_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from helpers import digest, make_inputs  # noqa: E402
from oracle import ref_harness  # noqa: E402

# tests/test_oracle.py::test_oracle_vs_live_reference
FORWARD_CASES = [(1, 228, 304, 12, "8sum", False), (2, 31, 45, 24, "8sum", True), (1, 64, 200, 24, "8sum_abs", True)]
NORMS = {0: "8sum", 1: "8sum_abs"}


def forward_key(B, H, W, N, norm, sp):
    return "forward/%d_%d_%d_%d_%s_%d/out" % (B, H, W, N, norm, int(sp))


def heads_inputs():
    """tests/test_head.py::test_head_oracle_vs_live_reference"""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, 64, 6, 5, generator=gen)
    w6, w5 = torch.randn(8, 64, 3, 3, generator=gen) * 0.05, torch.randn(1, 64, 3, 3, generator=gen) * 0.05
    return x, w6, w5


def heads_grad_inputs():
    """tests/test_head.py::test_head_backward_oracle_vs_live_reference"""
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(2, 6, 5, 7, generator=gen)
    w6 = torch.randn(8, 6, 3, 3, generator=gen)
    w5 = torch.randn(1, 6, 3, 3, generator=gen)
    gg, gb = torch.randn(2, 8, 9, 13, generator=gen), torch.randn(2, 1, 9, 13, generator=gen)
    return x, w6, w5, gg, gb


def prenorm_grad_inputs():
    """tests/test_backward.py::test_prenorm_backward_oracle_vs_live_reference"""
    gen = torch.Generator().manual_seed(31)
    g = torch.randn(1, 8, 7, 9, generator=gen)
    h = torch.rand(1, 1, 7, 9, generator=gen) * 5
    s = (torch.rand(1, 1, 7, 9, generator=gen) < 0.2).float() * 2.0
    go = torch.randn(1, 1, 7, 9, generator=gen)
    return g, h, s, go


def main():
    assert ref_harness.available(), "needs the reference tree"
    out = {}
    for B, H, W, N, norm, sp in FORWARD_CASES:
        g, h, s = make_inputs(B, H, W, seed=7, sparse=sp, neg=sp)
        out[forward_key(B, H, W, N, norm, sp)] = ref_harness.reference_forward(g, h, s, N, norm).numpy()
    rg, rb = ref_harness.reference_guidance_heads(*heads_inputs(), 12, 10)
    out["heads/guidance"], out["heads/blur"] = rg.detach().numpy(), rb.detach().numpy()
    dx, d6, d5 = ref_harness.reference_guidance_heads_grads(*heads_grad_inputs(), 9, 13)
    out["heads_grad/x"], out["heads_grad/w_guidance"], out["heads_grad/w_blur"] = dx.numpy(), d6.numpy(), d5.numpy()
    wb, o, gwb, gh = ref_harness.reference_grads_wrt_gate_wb(*prenorm_grad_inputs(), 5, "8sum_abs")
    out["prenorm_grad/gate_wb"], out["prenorm_grad/out"], out["prenorm_grad/grad_gate_wb"], out["prenorm_grad/grad_blur"] = (
        wb.numpy(), o.numpy(), gwb.numpy(), gh.numpy())
    path = os.path.join(HERE, "live_reference_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")

    digests = {"cspn2d_norm_golden.npz": {}, "aux_golden.npz": {}}
    src = np.load(os.path.join(HERE, "cspn2d_golden.npz"))
    norm_cases = sorted({k.split("/")[0] for k in np.load(os.path.join(HERE, "cspn2d_norm_golden.npz")).files})
    for name in norm_cases:
        wb, gs = ref_harness.reference_gate_wb(torch.from_numpy(src[name + "/guidance"]), NORMS[int(src[name + "/meta"][4])])
        digests["cspn2d_norm_golden.npz"][name + "/gate_wb"] = digest(wb.numpy())
        digests["cspn2d_norm_golden.npz"][name + "/gate_sum"] = digest(gs.numpy())
    import make_aux_golden
    with tempfile.TemporaryDirectory() as d:
        make_aux_golden.OUT = os.path.join(d, "aux.npz")
        make_aux_golden.main()
        z = np.load(make_aux_golden.OUT)
        for k in z.files:
            digests["aux_golden.npz"][k] = digest(z[k])
    path = os.path.join(HERE, "reference_digests.json")
    with open(path, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
