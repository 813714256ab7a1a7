"""Generates tests/golden/cspn2d_norm_grad_golden.npz: dL/dguidance as torch autograd computes it through the UNMODIFIED reference's
affinity_normalization (reference cspn_pytorch/models/cspn.py:85-144) for a seeded R = dL/dgate_wb, gate_wb cropped to the image
like the reference crops the product (cspn.py:72) -- the contract of cspn2d_normalize_backward_f32 (include/cspn_amd.h).

Cases: the guidance tensors of tests/golden/cspn2d_golden.npz that make_norm_golden.py uses (each with its own norm; the guidance is read
from there, only the new arrays are stored here), plus three stored with their guidance:
  k_edge_zeros_{8sum,abs}  values in {-1, -0.5, 0, 0.5, 1}, exact zeros next to the image edge and a pixel whose neighbourhood is all zero
                           (sign(0) and the edge; S = 0 gives NaN)
  m_wide_257_abs           257 columns (>= 256, W % 4 != 0)
R is a multiple of 1/16 in [-1, 1] (exact in float32, small on disk).

The reference normalises in the padded (H+2) x (W+2) frame.  A guidance element that no image pixel reads is read only by a pixel of the
padding ring, which the crop discards: its R is 0, so autograd gives 0 / S = 0 there -- or 0 / 0 = NaN where the ring pixel's neighbourhood
sums to zero (the k_edge_zeros cases have such ring pixels).  That NaN is the ONLY non-finite value on such elements (asserted below); the
engine writes 0 there (the convention of cspn2d_backward_f32), so tests compare those elements against 0, and everything else against the
stored values NaN for NaN.

Run where the reference tree is present (oracle/ref_harness.py loads it); the tests need only the result:
    python tests/golden/make_norm_grad_golden.py
The resulting .npz is committed; tests read it, never the reference tree."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.ref_harness import cuda_is_identity, load_reference_module  # noqa: E402

FROM_GOLDEN = ["a_8sum_sparse_neg", "b_abs_sparse", "d_row_1x7", "e_3x3", "f_1x1_nan", "g_zero_guidance_patch", "i_multiband_280",
               "j_col_9x1", "l_n30_abs"]
DY = [1, 1, 1, 0, 0, -1, -1, -1]
DX = [1, 0, -1, 1, -1, 1, 0, -1]


def reference_norm_grad(guidance, R, norm):
    """-> dL/dguidance of L = sum(gate_wb[..., image] * R) through the unmodified reference affinity_normalization"""
    ref = load_reference_module()
    m = ref.Affinity_Propagate(1, 3, norm)
    B, _, H, W = guidance.shape
    with cuda_is_identity():
        with torch.no_grad():
            m(guidance, torch.zeros(B, 1, H, W), None)           # creates m.sum_conv exactly as the reference does (cspn.py:44-53)
        g = guidance.clone().requires_grad_(True)
        wb, _ = m.affinity_normalization(g)
        gg, = torch.autograd.grad(wb[:, :, 0, 1:-1, 1:-1], g, R)
    return gg


def unread_mask(B, H, W):
    """[B,8,H,W] True where g_k(q) is read by no image pixel (q - off_k outside the image)"""
    m = np.zeros((B, 8, H, W), bool)
    y, x = np.mgrid[0:H, 0:W]
    for k in range(8):
        m[:, k] = ((y - DY[k] < 0) | (y - DY[k] >= H) | (x - DX[k] < 0) | (x - DX[k] >= W))[None]
    return m


def edge_case(seed):
    gen = torch.Generator().manual_seed(seed)
    g = (torch.randint(-2, 3, (1, 8, 6, 9), generator=gen) * 0.5).float()
    g[:, :, 0, :] *= (torch.rand(1, 8, 9, generator=gen) < 0.5).float()       # extra zeros on the edge rows / columns
    g[:, :, -1, :] *= (torch.rand(1, 8, 9, generator=gen) < 0.5).float()
    g[:, :, :, 0] *= (torch.rand(1, 8, 6, generator=gen) < 0.5).float()
    for k in range(8):                                                          # pixel (2, 4) reads nothing but zeros: S = 0
        g[:, k, 2 + DY[k], 4 + DX[k]] = 0.0
    return g


def main():
    src = np.load(os.path.join(HERE, "cspn2d_golden.npz"))
    cases = [(name, torch.from_numpy(src[name + "/guidance"]), "8sum_abs" if int(src[name + "/meta"][4]) else "8sum", False)
             for name in FROM_GOLDEN]
    cases += [("k_edge_zeros_8sum", edge_case(1), "8sum", True), ("k_edge_zeros_abs", edge_case(2), "8sum_abs", True)]
    gen = torch.Generator().manual_seed(3)
    cases += [("m_wide_257_abs", torch.randn(1, 8, 3, 257, generator=gen), "8sum_abs", True)]
    out = {}
    for i, (name, g, norm, store_guidance) in enumerate(cases):
        gen = torch.Generator().manual_seed(100 + i)
        R = torch.randint(-16, 17, g.shape, generator=gen).float() / 16
        gg = reference_norm_grad(g, R, norm).numpy()
        un = unread_mask(*g.shape[:1], *g.shape[2:])
        assert np.all((gg[un] == 0) | np.isnan(gg[un])), name          # unread elements: 0, or NaN from a ring pixel with S = 0
        if store_guidance:
            out[name + "/guidance"] = g.numpy()
        out[name + "/grad_wb"] = R.numpy()
        out[name + "/grad_guidance"] = gg.astype(np.float32)
        out[name + "/meta"] = np.array([int(norm == "8sum_abs")], np.int32)
        print(name, norm, tuple(g.shape), "nan read:", int(np.isnan(gg[~un]).sum()), "nan unread:", int(np.isnan(gg[un]).sum()))
    path = os.path.join(HERE, "cspn2d_norm_grad_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
