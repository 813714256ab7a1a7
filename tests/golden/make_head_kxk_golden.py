"""Generates tests/golden/head_kxk_golden.npz: what the UNMODIFIED reference class Simple_Gudi_UpConv_Block_Last_Layer
(/root/reference/cspn_pytorch/models/torch_resnet_cspn_nyu.py:187-206: Unpool :41-54 + bias-free 3x3 conv) returns when it is instantiated with 24 or 48
output planes -- the guidance head of cspn_config['kernel'] = 5 / 7 (K*K-1 planes; the class takes the plane count as an argument) -- next to the 1-plane blur
head (:318), for seeded inputs and weights, and the gradients torch autograd computes through both with respect to the feature map and the two conv weights
for a seeded output gradient.  Authoring container only (the reference tree is not on the GPU box):
    python tests/golden/make_head_kxk_golden.py
The resulting .npz is committed; tests read it, never /root/reference."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.ref_harness import cuda_is_identity, REF_MODEL  # noqa: E402

# name: (B, C, h, w, oheight, owidth)   (0, 0: no narrowing)
CASES = {
    "a_exact_2x": (2, 34, 3, 5, 6, 10),           # 34 channels: two 32-channel blocks of the backward kernels, the second partly filled
    "b_no_narrow": (1, 12, 5, 6, 0, 0),
    "c_narrow_odd": (1, 8, 2, 35, 3, 69),        # crosses a 32-column tile of the kernels; odd output sizes; the last input column feeds one output column
    "d_few_channels": (1, 5, 5, 4, 10, 8),
    "e_one_pixel": (1, 3, 1, 1, 2, 2),
    "f_narrow_more": (1, 8, 4, 10, 5, 17),       # the last input row / column lies beyond the narrowed output: no gradient reaches it
}


def reference_heads_and_grads(x, wg, wb, gg_fn, oh, ow):
    """the reference layers (wg.shape[0] guidance planes, 1 blur plane) on x: outputs, then autograd of sum(g * gg) + sum(b * gb)"""
    d = os.path.dirname(REF_MODEL)
    sys.path.insert(0, d)            # the file does `import cspn as post_process` (:12)
    try:
        with cuda_is_identity():
            spec = importlib.util.spec_from_file_location("_reference_resnet_cspn", REF_MODEL)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            C = x.shape[1]
            lg = mod.Simple_Gudi_UpConv_Block_Last_Layer(C, wg.shape[0], oh, ow)
            lb = mod.Simple_Gudi_UpConv_Block_Last_Layer(C, 1, oh, ow)
            with torch.no_grad():
                lg.conv1.weight.copy_(wg)
                lb.conv1.weight.copy_(wb)
            xr = x.clone().requires_grad_(True)
            g, b = lg(xr), lb(xr)
            gg, gb = gg_fn(g.shape), gg_fn(b.shape)
            (g * gg).sum().add((b * gb).sum()).backward()
            return g.detach(), b.detach(), gg, gb, xr.grad.detach(), lg.conv1.weight.grad.detach(), lb.conv1.weight.grad.detach()
    finally:
        sys.path.remove(d)


def main():
    out = {}
    for K in (5, 7):
        P = K * K - 1
        for name, (B, C, h, w, oh, ow) in CASES.items():
            gen = torch.Generator().manual_seed(sum(map(ord, name)) + 100 * K)
            x = torch.randn(B, C, h, w, generator=gen)
            wg = torch.randn(P, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)
            wb = torch.randn(1, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)
            g, b, gg, gb, dx, dwg, dwb = reference_heads_and_grads(x, wg, wb, lambda s: torch.randn(*s, generator=gen), oh, ow)
            key = "k%d_%s/" % (K, name)
            for k, v in (("x", x), ("wg", wg), ("wb", wb), ("guidance", g), ("blur", b), ("grad_guidance", gg), ("grad_blur", gb), ("grad_x", dx),
                         ("grad_wg", dwg), ("grad_wb", dwb)):
                out[key + k] = v.numpy()
            out[key + "meta"] = np.array([oh, ow, K], np.int32)
            print(key, tuple(g.shape), tuple(b.shape), float(dx.abs().max()), float(dwg.abs().max()), float(dwb.abs().max()))
    path = os.path.join(HERE, "head_kxk_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
