"""Generates tests/golden/head_norm_grad_golden.npz: the gradients torch autograd computes through the UNMODIFIED reference pipeline
    guidance = gud_up_proj_layer6(x); blur = gud_up_proj_layer5(x)          (torch_resnet_cspn_nyu.py:372-373, heads :187-206, Unpool :41-54)
    out = Affinity_Propagate(N, 3, norm)(guidance, blur, sparse)            (cspn.py:14-83, normalisation :85-144)
with respect to x and the two conv weights, for L = sum(out * grad_out) with a seeded grad_out, norm '8sum' and '8sum_abs'.  It pins the engine's
composed route guidance_heads(x, w6, w5, oh, ow, norm_type=norm) -> propagate_prenorm(gate_wb, blur, sparse, N) to the reference's own autograd.
Run where the reference tree is present (oracle/ref_harness.py loads it); the tests need only the result:
    python tests/golden/make_head_norm_grad_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.ref_harness import REF_MODEL, cuda_is_identity, load_reference_module  # noqa: E402

# name: (B, C, h, w, oheight, owidth, N, norm, sparse)
CASES = {
    "a_8sum_exact_2x": (2, 16, 6, 10, 12, 20, 12, "8sum", True),
    "b_abs_narrow_odd": (1, 8, 5, 70, 9, 139, 24, "8sum_abs", False),
    "c_8sum_narrow": (1, 8, 7, 33, 13, 64, 24, "8sum", True),
    "d_abs_exact_2x": (2, 16, 4, 9, 8, 18, 8, "8sum_abs", True),
}


def reference_grads(x, w6, w5, sparse, grad_out, oh, ow, n_iter, norm):
    d = os.path.dirname(REF_MODEL)
    sys.path.insert(0, d)   # the model file does `import cspn as post_process` (:12)
    try:
        with cuda_is_identity():
            spec = importlib.util.spec_from_file_location("_reference_resnet_cspn", REF_MODEL)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            C = x.shape[1]
            l6 = mod.Simple_Gudi_UpConv_Block_Last_Layer(C, 8, oh, ow)
            l5 = mod.Simple_Gudi_UpConv_Block_Last_Layer(C, 1, oh, ow)
            with torch.no_grad():
                l6.conv1.weight.copy_(w6)
                l5.conv1.weight.copy_(w5)
            prop = load_reference_module().Affinity_Propagate(n_iter, 3, norm)
            xr = x.clone().requires_grad_(True)
            out = prop(l6(xr), l5(xr), sparse)
            (out * grad_out).sum().backward()
            return out.detach(), xr.grad.detach(), l6.conv1.weight.grad.detach(), l5.conv1.weight.grad.detach()
    finally:
        sys.path.remove(d)


def main():
    out = {}
    for name, (B, C, h, w, oh, ow, N, norm, sp) in CASES.items():
        gen = torch.Generator().manual_seed(sum(map(ord, name)) + 11)
        x = torch.randn(B, C, h, w, generator=gen)
        w6 = torch.randn(8, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)
        w5 = torch.randn(1, C, 3, 3, generator=gen) / (3.0 * C ** 0.5) + 0.05
        sparse = (torch.rand(B, 1, oh, ow, generator=gen) < 0.05).float() * 2.0 if sp else None
        go = torch.randn(B, 1, oh, ow, generator=gen)
        o, dx, dw6, dw5 = reference_grads(x, w6, w5, sparse, go, oh, ow, N, norm)
        assert all(bool(torch.isfinite(t).all()) for t in (o, dx, dw6, dw5)), name
        for k, v in (("x", x), ("w6", w6), ("w5", w5), ("grad_out", go), ("out", o), ("grad_x", dx), ("grad_w6", dw6), ("grad_w5", dw5)):
            out[name + "/" + k] = v.numpy()
        if sparse is not None:
            out[name + "/sparse"] = sparse.numpy()
        out[name + "/meta"] = np.array([oh, ow, N, int(norm == "8sum_abs")], np.int32)
        print(name, norm, tuple(dx.shape), float(dx.abs().max()), float(dw6.abs().max()), float(dw5.abs().max()))
    path = os.path.join(HERE, "head_norm_grad_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
