"""GPU (MI355X): the HIP path, called through the C ABI, against the CPU oracle, the
committed golden vectors of the reference, and size-independent properties at
BASELINE.json's full sizes.  Tolerance: 1e-4 relative (BASELINE.json north_star)."""
import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from helpers import RTOL, assert_close, assert_close_tight, config_inputs, hand_mask, make_inputs, rel_err
from oracle import cspn2d_oracle, cspn3d_oracle

pytestmark = pytest.mark.gpu
NORMS = {0: "8sum", 1: "8sum_abs"}
DEV = "cuda:0"


def _algos(B, H, W, N):
    lib = cspn_amd.load()
    algos = ["stepwise"]
    if N > 0 and lib.cspn2d_auto_algo(B, H, W, N) == _lib.ALGOS["fused_padded"]:
        algos += ["fused_padded", "auto"]
    if N > 0 and lib.cspn2d_auto_algo(B, H, W, N) == _lib.ALGOS["fused"]:
        algos.append("fused")
        algos.append("fused_cxx")
        if N >= 24 and W >= 256 and W % 4 == 0:   # passes of 24 iterations run the assembly loop: also on the other plans
            algos += ["fused_groups", "fused_noxcd"]
    return algos


def _forward(g, h, s, N, norm, algo):
    """cspn2d_forward; 'fused_groups' / 'fused_noxcd' = algo 'fused' with the assembly passes on the band-group plan of rounds
    1-3 / on the linear plan without XCD-aware placement (hook library: the plan is an argument of an internal entry point)"""
    mode = {"fused_noxcd": 1, "fused_groups": 2, "fused_ring8": 8, "fused_ring12": 16, "fused_ring12_noxcd": 17}.get(algo)   # + 8 / + 16: the 8 x 4 / the 12 x 3 ring
    if mode is None:
        return cspn_amd.cspn2d_forward(g, h, s, N, norm, algo)
    hooks = _lib.load_hooks()
    B, _, H, W = g.shape
    out = torch.empty_like(h)
    ws = torch.empty(max(1, cspn_amd.load().cspn2d_workspace_bytes(B, H, W, N)), dtype=torch.uint8, device=g.device)
    st = torch.cuda.current_stream().cuda_stream
    rc = hooks.cspn_debug_forward2d_plan(g.data_ptr(), h.data_ptr(), s.data_ptr() if s is not None else None, out.data_ptr(), B, H, W, N,
                                         _lib.NORM_TYPES[norm], mode, ws.data_ptr(), st)
    _lib.check(rc, "cspn_debug_forward2d_plan")
    return out


def _run(g, h, s, N, norm, algo):
    out = _forward(g.to(DEV), h.to(DEV), None if s is None else s.to(DEV), N, norm, algo)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_library_is_loaded_and_gpu_present():
    assert torch.cuda.is_available()
    assert cspn_amd.load().cspn_abi_version() == 5


def test_golden_vectors(golden):
    for name, c in golden.items():
        B, H, W, N, norm = [int(v) for v in c["meta"]]
        g, h = torch.from_numpy(c["guidance"]), torch.from_numpy(c["blur"])
        s = torch.from_numpy(c["sparse"]) if "sparse" in c else None
        if N == 0:
            continue
        for algo in _algos(B, H, W, N):
            assert_close_tight(_run(g, h, s, N, NORMS[norm], algo), c["out"], "%s/%s" % (name, algo))


SHAPES = [
    # B, H, W, N, norm, sparse
    (1, 228, 304, 12, "8sum", False),      # BASELINE config 1 shape
    (2, 228, 304, 24, "8sum", True),       # config 2 shape (reduced batch; full batch below)
    (1, 304, 1216, 24, "8sum", True),      # KITTI shape
    (1, 304, 1216, 24, "8sum_abs", True),
    (2, 37, 53, 24, "8sum", True),         # odd sizes, W not a multiple of 4
    (1, 5, 300, 24, "8sum_abs", False),    # short and wide
    (1, 300, 6, 24, "8sum", True),         # tall and narrow
    (3, 64, 256, 7, "8sum", True),         # exactly one band wide
    (1, 65, 260, 24, "8sum", True),        # just over one band
    (1, 100, 516, 30, "8sum", True),       # n_iter > 24
    (1, 1, 1, 3, "8sum", False),           # 1x1 -> NaN (no in-range neighbour)
    (2, 2, 2, 2, "8sum_abs", True),
    (1, 40, 1216, 1, "8sum", True),
    (5, 48, 128, 24, "8sum", True),
    # the smallest images a per-pixel kernel can get wrong, two of them each (batch stride): one row, one column, non-square
    (2, 1, 5, 3, "8sum", False),
    (2, 4, 1, 3, "8sum_abs", True),
    (2, 3, 2, 3, "8sum", True),
]
HAND_MASKED = {(2, 4, 1), (2, 3, 2)}   # too small for make_inputs' 5 % mask (mostly empty there): helpers.hand_mask


@pytest.mark.parametrize("B,H,W,N,norm,sp", SHAPES)
def test_parity_vs_oracle(B, H, W, N, norm, sp):
    g, h, s = make_inputs(B, H, W, seed=B * 1000 + H + W + N, sparse=sp, neg=sp, depth_scale=80.0)
    if sp and (B, H, W) in HAND_MASKED:
        s = hand_mask(h, neg=True)
    ref = cspn2d_oracle(g, h, s, N, norm)
    for algo in _algos(B, H, W, N):
        assert_close_tight(_run(g, h, s, N, norm, algo), ref, algo)


def test_nan_semantics_zero_guidance():
    g, h, s = make_inputs(1, 40, 64, seed=9)
    g[:, :, 10:17, 20:29] = 0.0  # 0/0 at cspn.py:138
    ref = cspn2d_oracle(g, h, s, 3)
    assert np.isnan(ref).sum() > 0
    for algo in _algos(1, 40, 64, 3):
        assert rel_err(_run(g, h, s, 3, "8sum", algo), ref) <= RTOL


def test_module_call_and_stream_semantics():
    g, h, s = make_inputs(2, 60, 96, seed=21)
    m = cspn_amd.Affinity_Propagate(24, 3, "8sum").to(DEV)
    gd, hd, sd = g.to(DEV), h.to(DEV), s.to(DEV)
    g0, h0 = gd.clone(), hd.clone()
    with torch.no_grad():
        out = m(gd, hd, sd)
        out6 = m(gd, hd, sd, n_iter=6)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out_side = m(gd, hd, sd)
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert out.shape == (2, 1, 60, 96) and out.device == gd.device
    assert torch.equal(gd, g0) and torch.equal(hd, h0)  # inputs not mutated
    assert rel_err(out.cpu().numpy(), cspn2d_oracle(g, h, s, 24)) <= RTOL
    assert rel_err(out6.cpu().numpy(), cspn2d_oracle(g, h, s, 6)) <= RTOL
    assert torch.equal(out, out_side)  # deterministic, stream-agnostic
    assert list(m.state_dict().keys()) == []
    assert m(gd, hd, sd, n_iter=0) is hd


def test_noncontiguous_inputs():
    g, h, s = make_inputs(2, 33, 40, seed=4)
    gd = g.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # NHWC-strided view
    out = cspn_amd.cspn2d_forward(gd, h.to(DEV), s.to(DEV), 5)
    assert rel_err(out.cpu().numpy(), cspn2d_oracle(g, h, s, 5)) <= RTOL


# ---- BASELINE.json full sizes: oracle where it finishes in seconds, properties everywhere ----

def _pairwise_whole_batch(outs, name):
    """every HIP path agrees with every other on EVERY pixel of the batch (element-wise, on the device): the assembly
    loop, its compiler-generated twin and the one-launch-per-iteration path share no code beyond the fold arithmetic"""
    assert {"stepwise", "fused", "fused_cxx"} <= set(outs), sorted(outs)
    names = sorted(outs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            x, y = outs[a], outs[b]
            assert torch.equal(torch.isfinite(x), torch.isfinite(y)), (name, a, b)
            scale = float(y.abs().max())
            d = (x - y).abs()
            assert float(d.max()) <= RTOL * scale, (name, a, b, float(d.max()) / scale)
            # element-wise, with an absolute floor of 1e-6 of the largest depth (helpers.assert_close_tight)
            assert bool((d <= 1e-6 * scale + RTOL * y.abs()).all()), (name, a, b)


@pytest.mark.parametrize("name,B,H,W,scale,sparse", [("config2", 16, 228, 304, 10.0, True),
                                                     ("config3_per_gpu", 8, 304, 1216, 80.0, False),
                                                     ("config4", 32, 304, 1216, 80.0, True)])
def test_full_size_configs(name, B, H, W, scale, sparse):
    g, h, s = config_inputs(B, H, W, scale, sparse)
    gd, hd = g.to(DEV), h.to(DEV)
    sd = s.to(DEV) if sparse else None
    outs = {}
    for algo in _algos(B, H, W, 24):
        outs[algo] = _forward(gd, hd, sd, 24, "8sum", algo)
    torch.cuda.synchronize()
    # oracle on a sample of the batch (first, middle, last image)
    idx = sorted({0, B // 2, B - 1})
    ref = cspn2d_oracle(g[idx], h[idx], None if s is None else s[idx], 24, "8sum")
    for algo, out in outs.items():
        assert_close_tight(out[idx].cpu().numpy(), ref, "%s/%s" % (name, algo))
        # properties over the WHOLE batch
        if sparse:
            m = sd > 0
            assert torch.equal(out[m], hd[m])  # pinned pixels equal blur exactly (cspn.py:81)
        assert torch.isfinite(out).all()
        # linearity in the depth (fixed guidance/mask): f(2a - b/2) = 2 f(a) - f(b)/2
        h2 = torch.roll(hd, 1, 0)
        o2 = _forward(gd, h2, sd, 24, "8sum", algo)
        o12 = _forward(gd, 2.0 * hd - 0.5 * h2, sd, 24, "8sum", algo)
        lin = (o12 - (2.0 * out - 0.5 * o2)).abs().max() / out.abs().max()
        assert float(lin) <= RTOL, (name, algo, float(lin))
    _pairwise_whole_batch(outs, name)
    # constant depth is a fixed point
    const = torch.full_like(hd, 7.5)
    oc = cspn_amd.cspn2d_forward(gd, const, None, 24, "8sum_abs")
    assert float((oc - 7.5).abs().max()) <= 7.5 * RTOL


def _plan_info(B, H, W, mode=0, hist=0):
    import ctypes
    info = (ctypes.c_int * 8)()
    _lib.load_hooks().cspn_debug_tsw_plan_geo(B, H, W, mode, hist, info)
    return dict(zip(("kind", "n_wg", "stride", "kimg", "xcd", "per_xcd", "ng", "nb"), list(info)))


def _piece_edge_images(B, H, W):
    """global image indices that hold the first / last image row of every piece of the forward plan -- the places where a
    planner bug would show first"""
    import ctypes
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.tswgen.plan import LinearPlan
    lp = LinearPlan(B, H, W, 24, 256)
    idx = set()
    for p in range(lp.n_wg):
        for seg in lp.segments(lp.cut[p], lp.cut[p + 1]):
            idx.add(seg[0])
    cuts_mid_image = sorted({(lp.runs(c, c + 1)[0][1]) // H for c in lp.cut[1:-1] if c < lp.total and lp.runs(c, c + 1)[0][1] % H})
    return sorted(idx), cuts_mid_image, lp


@pytest.mark.parametrize("sparse", [False, True])
def test_benchmarked_shape_b64(sparse):
    """the very launch bench.py times (BASELINE config 3 at 64 images on one GPU: the linear plan, 256 pieces of 1.5 (image, band)
    units, XCD-aware placement), and config 4's mask at that batch: sampled oracle incl. images that are cut mid-image and the
    image whose bands the last four CUs share, all HIP paths and plans equal on the whole batch, masked pixels exact."""
    B, H, W = 64, 304, 1216
    g, h, s = config_inputs(B, H, W, 80.0, sparse)
    gd, hd = g.to(DEV), h.to(DEV)
    sd = s.to(DEV) if sparse else None
    outs = {a: _forward(gd, hd, sd, 24, "8sum", a) for a in ("stepwise", "fused", "fused_cxx", "fused_groups", "fused_noxcd", "fused_ring8", "fused_ring12")}
    torch.cuda.synchronize()   # ("fused" = the dispatcher's choice: round 6's 12 x 3 ring at this stream length; both rings explicitly)
    _pairwise_whole_batch(outs, "b64")
    info = _plan_info(B, H, W)
    assert info["kind"] == 1 and info["n_wg"] == 256 and info["xcd"] == 1 and info["kimg"] == 3, info   # the plan DESIGN.md describes
    assert info["stride"] == 481 + 36 + 48, info                                                          # 481 stream rows per CU
    _, mid, lp = _piece_edge_images(B, H, W)
    assert len(mid) >= 20                     # every second image is cut in the middle
    sample = sorted({0, 1, 31, 62, 63} | set(mid[::4]))   # first / last images (63: bands shared by the last 4 CUs) + cut images
    assert len(sample) >= 8
    ref = cspn2d_oracle(g[sample], h[sample], None if s is None else s[sample], 24, "8sum")
    for a, o in outs.items():
        assert_close_tight(o[sample].cpu().numpy(), ref, "b64/%s" % a)
        assert torch.isfinite(o).all()
        if sparse:
            m = sd > 0
            assert int(m.sum()) > 25000
            assert torch.equal(o[m], hd[m])


# ---- 3D ----

@pytest.mark.parametrize("B,D,H,W,N,norm,sp", [(1, 4, 9, 11, 5, "8sum_abs", False), (2, 6, 10, 37, 12, "8sum", True),
                                               (1, 3, 8, 64, 3, "none", False), (1, 1, 1, 1, 2, "8sum", False),
                                               (2, 5, 7, 12, 12, "none", False),   # direct kernel, ping-pong over 12 launches
                                               (1, 2, 5, 10, 2, "none", False),    # W % 4 != 0: general path
                                               (1, 4, 6, 16, 3, "none", True),     # sparse pins: general path
                                               (1, 1, 1, 4, 3, "none", False),     # one quad is the volume: no neighbour row inside it
                                               (2, 1, 2, 3, 3, "none", False),     # the one-voxel kernels at B = 2, every z-neighbour outside
                                               (2, 4, 5, 7, 3, "8sum", True)])     # folded step: batch and plane strides both differ from V
def test_3d_parity_vs_oracle(B, D, H, W, N, norm, sp):
    gen = torch.Generator().manual_seed(D * 100 + H)
    g = torch.randn(B, 26, D, H, W, generator=gen) if norm == "8sum" else torch.rand(B, 26, D, H, W, generator=gen)
    if norm == "none":
        g = g / g.sum(1, keepdim=True)  # cspn_paddle/demo.py:47-49
    h = torch.rand(B, 1, D, H, W, generator=gen)
    s = None
    if sp:
        s = (torch.rand(B, 1, D, H, W, generator=gen) < 0.05).float() * h
    out = cspn_amd.cspn3d_forward(g.to(DEV), h.to(DEV), None if s is None else s.to(DEV), N, norm)
    assert rel_err(out.cpu().numpy(), cspn3d_oracle(g, h, s, N, norm)) <= RTOL


def test_3d_config5_shape_properties():
    """BASELINE config 5: 32x160x608, batch 4, 12 iters, demo-style non-negative gates."""
    B, D, H, W = 4, 32, 160, 608
    gen = torch.Generator(device=DEV).manual_seed(5)
    g = torch.rand(B, 26, D, H, W, generator=gen, device=DEV)
    h = torch.rand(B, 1, D, H, W, generator=gen, device=DEV)
    out = cspn_amd.cspn3d_forward(g, h, None, 12, "8sum_abs")
    assert torch.isfinite(out).all()
    # convex combination of neighbours: stays inside the input range
    assert float(out.min()) >= -1e-5 and float(out.max()) <= 1.0 + 1e-5
    const = torch.full_like(h, 3.0)
    oc = cspn_amd.cspn3d_forward(g, const, None, 12, "8sum_abs")
    assert float((oc - 3.0).abs().max()) <= 3.0 * RTOL
    # oracle on one image at reduced depth would change the problem; instead check one sub-volume
    # against the oracle by running both on an identical smaller crop
    gc, hc = g[:1, :, :6, :24, :40].contiguous(), h[:1, :, :6, :24, :40].contiguous()
    oc = cspn_amd.cspn3d_forward(gc, hc, None, 12, "8sum_abs")
    assert rel_err(oc.cpu().numpy(), cspn3d_oracle(gc.cpu(), hc.cpu(), None, 12, "8sum_abs")) <= RTOL
    # the Paddle contract at full size (gates normalised by the caller, used as given): direct one-pass-per-step kernel
    gn = g / g.sum(1, keepdim=True)
    on = cspn_amd.cspn3d_forward(gn, h, None, 12, "none")
    assert float(on.min()) >= -1e-5 and float(on.max()) <= 1.0 + 1e-5
    # no centre term in this mode: mass leaks through the zero border, 12 voxels deep; the interior keeps a constant
    oc = cspn_amd.cspn3d_forward(gn, const, None, 12, "none")[:, :, 12:-12, 12:-12, 12:-12]
    assert float((oc - 3.0).abs().max()) <= 3.0 * RTOL
    gc = gn[1:2, :, :6, :24, :40].contiguous()
    oc = cspn_amd.cspn3d_forward(gc, hc, None, 12, "none")
    assert rel_err(oc.cpu().numpy(), cspn3d_oracle(gc.cpu(), hc.cpu(), None, 12, "none")) <= RTOL


@pytest.mark.parametrize("B,D,H,W,N", [(1, 8, 8, 64, 2),        # one tile, two steps
                                       (2, 20, 30, 200, 12),    # several tiles in z, y and x; ragged extents; two volumes
                                       (1, 32, 160, 304, 4),    # config-5 cross-section, two chunks along x (halo recomputation at the cut)
                                       (1, 32, 160, 152, 3),    # config-5 cross-section: 80 tile columns, 3 x-tiles per chunk
                                       (2, 10, 9, 68, 4)])      # W % 8 == 4: the volume ends inside a thread's first quad
def test_3d_persistent_vs_stepwise_and_oracle(B, D, H, W, N):
    """the persistent kernel (gates resident in registers across the steps, neighbour flags between tiles, chunks with
    n_iter halo) against the one-launch-per-step kernel on every voxel, and against the 3D oracle where that is quick"""
    gen = torch.Generator(device=DEV).manual_seed(D * 1000 + H + W)
    g = torch.rand(B, 26, D, H, W, generator=gen, device=DEV)
    g = g / g.sum(1, keepdim=True)
    h = torch.rand(B, 1, D, H, W, generator=gen, device=DEV)
    a, ws = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent", _return_ws=True)
    b = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="stepwise")
    torch.cuda.synchronize()
    assert _lib.load_hooks().cspn_debug_3d_persistent_error(ws.data_ptr(), B, D, H, W) == 0
    assert torch.isfinite(a).all()
    d = (a - b).abs()
    assert float(d.max()) <= 1e-5 * float(b.abs().max()), float(d.max())
    assert torch.equal(a, cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent"))   # deterministic
    if B * D * H * W <= 400000:
        assert_close(a.cpu().numpy(), cspn3d_oracle(g.cpu(), h.cpu(), None, N, "none"), "3d persistent")


@pytest.mark.parametrize("B,C,D,H,W,N", [(1, 3, 16, 24, 128, 6), (2, 2, 10, 9, 68, 4), (1, 3, 32, 160, 152, 12), (3, 4, 8, 16, 64, 2),
                                         (8, 3, 32, 160, 608, 4)])   # a wide row of volumes: several chunks per launch (the gates of the
                                                                     # NEXT chunk are parked during channel 0 only)
def test_3d_shared_gates_multi_channel_equals_per_channel_loop(B, C, D, H, W, N):
    """round 4: C input channels on shared gates (reference cspn_paddle/README.md:56) in ONE persistent launch -- the gates of a chunk
    are loaded once and stay in the registers while the steps run for channel after channel -- against C single-channel calls,
    bit for bit; cspn_amd.affinity_propagate takes that path for C > 1"""
    gen = torch.Generator(device=DEV).manual_seed(B * 100 + C * 10 + N)
    g = torch.rand(B, 26, D, H, W, generator=gen, device=DEV)
    g /= g.sum(1, keepdim=True)
    x = torch.rand(B, C, D, H, W, generator=gen, device=DEV) * 80
    assert cspn_amd.load().cspn3d_multi_supported(B, C, D, H, W, N)
    got = cspn_amd.cspn3d_forward_multi(g, x, N)
    ref = torch.cat([cspn_amd.cspn3d_forward(g, x[:, c:c + 1].contiguous(), None, N, "none", algo="persistent") for c in range(C)], 1)
    cspn_amd.cspn3d_check_status()
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref)
    with torch.no_grad():
        assert torch.equal(cspn_amd.affinity_propagate(x, g, 3, N), ref)
    if B * D * H * W <= 100000:
        assert_close(got[:, 1:2].cpu().numpy(), cspn3d_oracle(g.cpu(), x[:, 1:2].cpu(), None, N, "none"), "3d multi, channel 1")


def test_3d_config5_full_size_persistent_vs_stepwise_every_voxel():
    """BASELINE config 5 exactly (4 x 32x160x608, 12 steps): the geometry bench.py --workload vol3d times -- 15 chunks cut from
    the row of four volumes standing side by side -- against one launch per step, on every voxel.  Parity unpinned (the Paddle
    op's source is not in the reference tree): the two HIP paths hold each other, the oracle holds both on sub-volumes."""
    B, D, H, W, N = 4, 32, 160, 608, 12
    gen = torch.Generator(device=DEV).manual_seed(55)
    g = torch.rand(B, 26, D, H, W, generator=gen, device=DEV)
    g /= g.sum(1, keepdim=True)
    h = torch.rand(B, 1, D, H, W, generator=gen, device=DEV) * 80
    a, ws = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent", _return_ws=True)
    b = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="stepwise")
    cspn_amd.cspn3d_check_status()
    assert _lib.load_hooks().cspn_debug_3d_persistent_error(ws.data_ptr(), B, D, H, W) == 0
    assert torch.isfinite(a).all()
    d = (a - b).abs()
    tol = 1e-6 * float(b.abs().max()) + 1e-5 * b.abs()
    assert bool((d <= tol).all()), float(d.max())
    # round 5: an INDEPENDENT implementation on a whole volume -- the CPU oracle on all 3.1 M voxels of volume 1 (the chunks are
    # cut across the row of volumes, so volume 1 sees chunk cuts, a volume seam on both sides and every tile position)
    ref1 = cspn3d_oracle(g[1:2].cpu(), h[1:2].cpu(), None, N, "none")
    assert_close(a[1:2].cpu().numpy(), ref1, "3d persistent, full 32x160x608 volume vs the CPU oracle")
    assert_close(b[1:2].cpu().numpy(), ref1, "3d stepwise, full 32x160x608 volume vs the CPU oracle")
    del a, b, d, tol, ref1
    sub = (slice(1, 2), slice(None), slice(0, 8), slice(40, 64), slice(544, 608))   # a corner of volume 1 incl. its last columns
    gs, hs = g[sub].contiguous(), h[sub[0], :, sub[2], sub[3], sub[4]].contiguous()
    o = cspn_amd.cspn3d_forward(gs, hs, None, N, "none", algo="persistent")
    assert_close(o.cpu().numpy(), cspn3d_oracle(gs.cpu(), hs.cpu(), None, N, "none"), "3d persistent sub-volume")


def test_3d_persistent_timeout_surfaces_as_an_error():
    """a workgroup whose neighbour never publishes (test hook: one tile computes but keeps quiet -- what a tile that never got a
    compute unit looks like to the others) must not hang, must not return something that passes for a result, and must be
    reported: NaN in the output, CSPN_E_ASYNC from cspn3d_check_status and -- once -- from the next cspn3d_* call, after which the
    engine works again."""
    B, D, H, W, N = 1, 16, 24, 128, 6
    gen = torch.Generator(device=DEV).manual_seed(3)
    g = torch.rand(B, 26, D, H, W, generator=gen, device=DEV)
    g /= g.sum(1, keepdim=True)
    h = torch.rand(B, 1, D, H, W, generator=gen, device=DEV)
    good = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent")
    cspn_amd.cspn3d_check_status()
    hooks = _lib.load_hooks()
    ws = torch.empty(cspn_amd.load().cspn3d_workspace_bytes_ex(B, D, H, W, N, 2, 0), dtype=torch.uint8, device=DEV)

    def muted(wg):   # the persistent launch with workgroup wg keeping quiet (an argument of the hook entry point: no state anywhere)
        out = torch.empty_like(h)
        rc = hooks.cspn_debug_3d_persistent_forward(g.data_ptr(), h.data_ptr(), out.data_ptr(), B, D, H, W, N, wg, 0, ws.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return out
    bad = muted(1)                                                             # returns at once: the failure happens on the device
    with pytest.raises(cspn_amd.CspnError, match="gave up"):
        cspn_amd.cspn3d_check_status()
    assert bool(torch.isnan(bad).any())
    cspn_amd.cspn3d_check_status()                                             # reported once ...
    ok = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent")     # ... also when the OTHER workgroups of that launch
    cspn_amd.cspn3d_check_status()                                             # raised the word again after the report (launch numbers)
    assert torch.equal(ok, good)
    muted(0)
    torch.cuda.synchronize()
    with pytest.raises(cspn_amd.CspnError, match="gave up"):                   # the NEXT call finds it without a synchronisation
        cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent")
    again = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent")
    cspn_amd.cspn3d_check_status()
    assert torch.equal(again, good)


def _geo3(B, D, H, W, N):
    import ctypes
    info = (ctypes.c_int * 9)()
    _lib.load_hooks().cspn_debug_3d_geo(B, D, H, W, N, info)
    return dict(zip(("tz", "ty", "cx", "tiles", "launched", "bz", "by", "bx", "chunks"), list(info)))


@pytest.mark.parametrize("B,D,H,W,N", [(4, 32, 160, 608, 12), (1, 32, 160, 152, 6), (2, 16, 64, 200, 5), (1, 64, 64, 128, 3)])
def test_3d_xcd_aware_placement_is_bitwise_the_plain_order(B, D, H, W, N):
    """round 5: blocks of the tile grid go to workgroup ids that share an XCD, and a boundary row all of whose readers published the
    same XCC is stored L2-resident instead of write-through.  Placement and store scope change no arithmetic: the launch is bit for
    bit the plain-order launch (hook: same kernel, tiles in workgroup order, every neighbour then on another XCD)."""
    geo = _geo3(B, D, H, W, N)
    assert geo["bz"] > 0 and geo["launched"] == 8 * geo["bz"] * geo["by"] * geo["bx"] and geo["launched"] >= geo["tiles"], geo
    if (B, D, H, W) == (4, 32, 160, 608):
        assert (geo["tz"], geo["ty"], geo["cx"], geo["bz"], geo["by"], geo["bx"]) == (4, 20, 3, 2, 5, 3), geo   # config 5: 8 blocks of 30 tiles
    gen = torch.Generator(device=DEV).manual_seed(B + D + W)
    g = torch.rand(B, 26, D, H, W, generator=gen, device=DEV)
    g /= g.sum(1, keepdim=True)
    h = torch.rand(B, 1, D, H, W, generator=gen, device=DEV) * 80
    a = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent")
    cspn_amd.cspn3d_check_status()
    hooks = _lib.load_hooks()
    ws = torch.empty(cspn_amd.load().cspn3d_workspace_bytes_ex(B, D, H, W, N, 2, 0), dtype=torch.uint8, device=DEV)
    b = torch.empty_like(h)
    rc = hooks.cspn_debug_3d_persistent_forward(g.data_ptr(), h.data_ptr(), b.data_ptr(), B, D, H, W, N, -1, 2, ws.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    cspn_amd.cspn3d_check_status()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # the placement with EVERY published row write-through (hook bit 2): the L2-resident stores rest on a plain store
    # reaching the XCD's L2 in time for the neighbours' sc1 polls -- the pure write-through configuration must give the same bits
    c = torch.empty_like(h)
    rc = hooks.cspn_debug_3d_persistent_forward(g.data_ptr(), h.data_ptr(), c.data_ptr(), B, D, H, W, N, -1, 4, ws.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    cspn_amd.cspn3d_check_status()
    assert torch.equal(a, c)
    assert torch.equal(a, cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent"))   # and deterministic
    s = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="stepwise")
    assert float((a - s).abs().max()) <= 1e-5 * float(s.abs().max())


def test_3d_persistent_timeout_with_xcd_placement():
    """the loud-failure contract (NaN + CSPN_E_ASYNC) on a launch that uses the XCD-aware placement: a muted tile in the middle of a
    block (its rows would have been L2-resident) and one at a block face"""
    B, D, H, W, N = 1, 32, 160, 152, 4
    geo = _geo3(B, D, H, W, N)
    assert geo["bz"] > 0
    gen = torch.Generator(device=DEV).manual_seed(4)
    g = torch.rand(B, 26, D, H, W, generator=gen, device=DEV)
    g /= g.sum(1, keepdim=True)
    h = torch.rand(B, 1, D, H, W, generator=gen, device=DEV)
    good = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent")
    cspn_amd.cspn3d_check_status()
    hooks = _lib.load_hooks()
    ws = torch.empty(cspn_amd.load().cspn3d_workspace_bytes_ex(B, D, H, W, N, 2, 0), dtype=torch.uint8, device=DEV)
    for tile in ((0 * geo["ty"] + 2) * geo["cx"] + 1, (1 * geo["ty"] + 4) * geo["cx"] + 0):
        out = torch.empty_like(h)
        rc = hooks.cspn_debug_3d_persistent_forward(g.data_ptr(), h.data_ptr(), out.data_ptr(), B, D, H, W, N, tile, 0, ws.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        with pytest.raises(cspn_amd.CspnError, match="gave up"):
            cspn_amd.cspn3d_check_status()
        assert bool(torch.isnan(out).any())
        again = cspn_amd.cspn3d_forward(g, h, None, N, "none", algo="persistent")
        cspn_amd.cspn3d_check_status()
        assert torch.equal(again, good)


def test_paddle_style_affinity_propagate():
    gen = torch.Generator().manual_seed(8)
    x = torch.rand(2, 3, 5, 12, 16, generator=gen)  # C=3 channels share the gates (README.md:56)
    g = torch.rand(2, 26, 5, 12, 16, generator=gen)
    g = g / g.sum(1, keepdim=True)
    out = cspn_amd.affinity_propagate(x.to(DEV), g.to(DEV), kernel_size=3)
    assert out.shape == x.shape
    for c in range(3):
        ref = cspn3d_oracle(g, x[:, c:c + 1], None, 1, "none")
        assert rel_err(out[:, c:c + 1].cpu().numpy(), ref) <= RTOL
    x2 = torch.rand(2, 1, 20, 24, generator=gen)
    g2 = torch.rand(2, 8, 20, 24, generator=gen)
    g2 = g2 / g2.sum(1, keepdim=True)
    o2 = cspn_amd.affinity_propagate(x2.to(DEV), g2.to(DEV), n_iter=4)
    assert rel_err(o2.cpu().numpy(), cspn2d_oracle(g2, x2, None, 4, "none")) <= RTOL


# ---- shapes that take the assembly main loop (cspn2d_tsw.hip: W >= 256; round 5: any n_iter = a short first pass + full passes) ------
TSW_SHAPES = [
    (2, 40, 256, 24, "8sum", True),        # one band, both band-edge flags on the same band
    (1, 70, 512, 24, "8sum", False),       # two bands, the last one shifted to the image edge
    (3, 33, 304, 24, "8sum_abs", True),    # NYU width: bands at 0 and 48; several images per workgroup share
    (1, 3, 260, 24, "8sum", True),         # fewer rows than iterations
    (1, 1, 256, 24, "8sum", False),        # single row: both vertical neighbours missing
    (2, 50, 300, 48, "8sum", True),        # two assembly passes chained through the ping buffer
    (1, 64, 516, 30, "8sum_abs", True),    # a short first pass of 6 + a full pass (round 5; fused_cxx: 24 + 6 in the compiler-generated kernel)
    (2, 50, 300, 12, "8sum", True),        # BASELINE config 1's count: one short pass
    (1, 40, 260, 1, "8sum", False),        # a single iteration
    (2, 37, 304, 23, "8sum_abs", True),    # the longest short pass
    (1, 33, 520, 59, "none", True),        # 11 + 24 + 24
    (1, 45, 1216, 24, "none", True),       # KITTI width, centre-sited pre-normalised gates
    (6, 304, 1216, 24, "8sum", True),      # full-size images, every workgroup on the device busy
]


@pytest.mark.parametrize("B,H,W,N,norm,sp", TSW_SHAPES)
def test_asm_loop_parity_vs_oracle(B, H, W, N, norm, sp):
    g, h, s = make_inputs(B, H, W, seed=7 * B + H + W + N, sparse=sp, neg=sp, depth_scale=80.0)
    if norm == "none":
        g = g.abs() / (g.abs().sum(1, keepdim=True) + 0.25)
    if H > 20:
        g[0, :, 9:12, 100:108] = 0.0  # 0/0 -> NaN patch must spread exactly like the reference's (cspn.py:138)
    ref = cspn2d_oracle(g, h, s, N, norm)
    outs = {a: _run(g, h, s, N, norm, a) for a in ("fused", "fused_cxx", "fused_groups", "fused_noxcd", "fused_ring8", "fused_ring12", "fused_ring12_noxcd")}
    for a, o in outs.items():   # (round 6: full first passes on both rings, whichever the dispatcher would pick for the shape)
        assert_close_tight(o, ref, a)


@pytest.mark.parametrize("B,H,W,N,norm,sp", [(2, 41, 302, 24, "8sum", True),       # W % 4 = 2: assembly loop on 304-column rows
                                             (1, 30, 1217, 24, "8sum_abs", False),  # W % 4 = 1, several bands
                                             (3, 37, 259, 30, "8sum", True),        # W % 4 = 3: 256 real columns + 3; short pass + full pass (ping buffer)
                                             (2, 19, 50, 7, "8sum", True),          # narrow: the compiler-generated kernel on 52 columns
                                             (2, 33, 301, 24, "none", True),        # gates used as given: copied, not normalised
                                             (1, 25, 270, 12, "prenorm", False)])
def test_width_not_a_multiple_of_four_takes_the_padded_fused_path(B, H, W, N, norm, sp):
    """round 5: W % 4 != 0 ran fold + one launch per iteration (4.85 ms at 304 x 1218 x 64 against 0.28 for 304 x 1216).  AUTO now lays the
    inputs out with rows padded to a multiple of 4 columns (zeros; 8sum / 8sum_abs normalised on the way, for the REAL width) and runs the
    fused path on those: the pad columns must behave exactly like the reference's zero padding outside the image -- NaN patch (0/0),
    negative-sparse points and the right image edge included"""
    assert cspn_amd.load().cspn2d_auto_algo(B, H, W, N) == _lib.ALGOS["fused_padded"]
    g, h, s = make_inputs(B, H, W, seed=B + H + W + N, sparse=sp, neg=sp, depth_scale=80.0)
    g[0, :, 9:12, W - 9:W - 2] = 0.0      # zero guidance next to the right edge: 0/0 -> NaN must spread exactly as in the reference
    gr = g
    if norm == "none":
        g = g.abs() / (g.abs().sum(1, keepdim=True) + 0.25)
        ref = cspn2d_oracle(g, h, s, N, "none")
    elif norm == "prenorm":
        from oracle.oracle import cspn2d_gate_wb_oracle
        ref = cspn2d_oracle(gr, h, s, N, "8sum")
        g = torch.from_numpy(cspn2d_gate_wb_oracle(gr.numpy(), "8sum"))
    else:
        ref = cspn2d_oracle(g, h, s, N, norm)
    for algo in ("auto", "fused_padded", "stepwise"):
        o = _run(g, h, s, N, norm, algo)
        assert_close_tight(o, ref, algo)
    # explicit FUSED stays an error for such a width (the caller asked for a kernel that cannot take it)
    with pytest.raises(Exception):
        _run(g, h, s, N, norm, "fused")


def test_asm_loop_every_iteration_count_matches_the_compiled_kernel():
    """round 5: n_iter = 1 .. 50 all run in the assembly loop (a short first pass of n_iter % 24 iterations -- the row is stored when it
    completes that level --, then full passes); against the compiler-generated ring kernel, which plans and retires independently, and
    for a few counts against the oracle; NaN patch and negative-sparse points included"""
    B, H, W = 3, 61, 304
    g, h, s = make_inputs(B, H, W, seed=4242, sparse=True, neg=True, depth_scale=80.0)
    g[1, :, 20:23, 100:108] = 0.0
    for n in range(1, 51):
        for norm in (("8sum",) if n % 5 else ("8sum", "8sum_abs")):
            a = _run(g, h, s if n % 2 else None, n, norm, "fused")
            b = _run(g, h, s if n % 2 else None, n, norm, "fused_cxx")
            assert np.array_equal(np.isnan(a), np.isnan(b)), (n, norm)
            assert rel_err(a, b) <= 1e-5, (n, norm, rel_err(a, b))
            if n in (1, 7, 12, 23, 25, 47):
                assert_close_tight(a, cspn2d_oracle(g, h, s if n % 2 else None, n, norm), "n_iter %d" % n)


@pytest.mark.parametrize("B,H,W,norm,sp", [(2, 40, 256, "8sum", True), (1, 70, 516, "8sum_abs", False), (3, 33, 304, "none", True),
                                           (4, 304, 1216, "8sum", True)])
def test_sited8_entry_point_vs_oracle(B, H, W, norm, sp):
    """SURVEY 8f-2 experiment: the additional entry point that takes the guidance in the producer-side layout
    ([B,H,W/2,8,2], gathered by cspn2d_guidance_to_sited8_f32) against the oracle on the ORIGINAL tensors, and bit for bit
    against the planar entry point (same loop, same arithmetic, only the loads differ)"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.tswgen.run_emu import sited8
    if not _lib.load_hooks().cspn_debug_sited8_supported(B, H, W, 24):
        pytest.skip("the sited8 experiment (closed, DESIGN.md 3.6) is only in experiment builds: make -C cspn_amd/csrc EXPERIMENTS=1")
    g, h, s = make_inputs(B, H, W, seed=3 * B + H + W, sparse=sp, neg=sp, depth_scale=80.0)
    if norm == "none":
        g = g.abs() / (g.abs().sum(1, keepdim=True) + 0.25)
    elif H > 20:
        g[0, :, 9:12, 100:108] = 0.0
    gd = g.to(DEV)
    g8 = cspn_amd.guidance_to_sited8(gd, norm)
    assert np.array_equal(g8.cpu().numpy(), sited8(g.numpy(), {"8sum": 0, "8sum_abs": 1, "none": 2}[norm]))   # the layout kernel
    out = cspn_amd.cspn2d_forward_sited8(g8, h.to(DEV), None if s is None else s.to(DEV), 24, norm)
    planar = cspn_amd.cspn2d_forward(gd, h.to(DEV), None if s is None else s.to(DEV), 24, norm, "fused")
    torch.cuda.synchronize()
    nz = ~torch.isnan(planar)
    # (the planar entry point streams the pieces of the linear plan, this one the band groups: same arithmetic, another summation order)
    assert torch.equal(torch.isnan(out), torch.isnan(planar))
    assert float((out[nz] - planar[nz]).abs().max()) <= 4e-6 * float(planar[nz].abs().max())
    if B * H * W <= 200000:
        assert_close_tight(out.cpu().numpy(), cspn2d_oracle(g, h, s, 24, norm), "sited8")
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.cspn2d_forward_sited8(g8, h.to(DEV), None, 12, norm)   # only whole 24-iteration passes

# ---- SURVEY 8f-2, second alternative: the normalisation done by the producer (CSPN_NORM_PRENORM, cspn2d_normalize_f32) ----------------
def test_normalize_kernel_and_prenorm_forward_vs_golden(golden, norm_golden):
    """the contract is the reference's own intermediate gate_wb (cspn.py:85-144).  (1) cspn2d_normalize_f32 reproduces the golden
    gate_wb the unmodified reference returned (NaN pattern included); (2) every HIP path, fed the GOLDEN gate_wb with norm 'prenorm',
    reproduces the golden outputs."""
    for name, n in norm_golden.items():
        c = golden[name]
        B, H, W, N, norm = [int(v) for v in c["meta"]]
        g = torch.from_numpy(c["guidance"]).to(DEV)
        wb = cspn_amd.cspn2d_normalize(g, NORMS[norm]).cpu().numpy()
        assert np.array_equal(np.isnan(wb), np.isnan(n["gate_wb"])), name
        fin = ~np.isnan(wb)
        assert not fin.any() or np.abs(wb[fin] - n["gate_wb"][fin]).max() <= 2e-6, name     # |w| <= 1: the reference's conv sums in another order
        s = torch.from_numpy(c["sparse"]) if "sparse" in c else None
        for algo in _algos(B, H, W, N):
            out = _run(torch.from_numpy(n["gate_wb"]), torch.from_numpy(c["blur"]), s, N, "prenorm", algo)
            assert_close_tight(out, c["out"], "%s/prenorm/%s" % (name, algo))


@pytest.mark.parametrize("B,H,W,N,norm,sp", [(2, 60, 304, 24, "8sum", True), (1, 304, 1216, 24, "8sum_abs", True), (3, 33, 516, 48, "8sum", False),
                                             (1, 64, 516, 30, "8sum", True), (2, 37, 53, 24, "8sum", True), (1, 100, 260, 7, "8sum_abs", False),
                                             (6, 304, 1216, 24, "8sum", True)])
def test_prenorm_contract_vs_oracle_on_the_original_tensors(B, H, W, N, norm, sp):
    """normalise on the device (the stand-alone producer epilogue), run the forward with norm 'prenorm' on every path, compare with
    the oracle on the ORIGINAL guidance; plus bit-level: the assembly loop's prenorm variant against its raw-guidance variant (the only
    difference is v_rcp_f32 x multiply vs an IEEE division: <= 3e-6 of the largest depth)"""
    g, h, s = make_inputs(B, H, W, seed=3 * B + H + W + N, sparse=sp, neg=sp, depth_scale=80.0)
    if H > 20:
        g[0, :, 9:12, 100:108] = 0.0   # NaN weights travel through the prenormalised tensor as they do through the raw one
    ref = cspn2d_oracle(g, h, s, N, norm)
    gd, hd, sd = g.to(DEV), h.to(DEV), None if s is None else s.to(DEV)
    wb = cspn_amd.cspn2d_normalize(gd, norm)
    assert_close(wb.cpu().numpy(), __import__("oracle").cspn2d_gate_wb_oracle(g, norm), "gate_wb", rtol=1e-5, atol_frac=1e-6)
    for algo in _algos(B, H, W, N):
        out = _forward(wb, hd, sd, N, "prenorm", algo)
        torch.cuda.synchronize()
        assert_close_tight(out.cpu().numpy(), ref, "prenorm/" + algo)
    raw = _forward(gd, hd, sd, N, norm, "auto")
    pre = _forward(wb, hd, sd, N, "prenorm", "auto")
    nz = ~torch.isnan(raw)
    assert torch.equal(torch.isnan(raw), torch.isnan(pre))
    assert float((raw[nz] - pre[nz]).abs().max()) <= 3e-6 * float(raw[nz].abs().max())
    # through the dedicated entry point
    lib = cspn_amd.load()
    out2 = torch.empty_like(hd)
    ws_bytes = lib.cspn2d_workspace_bytes(B, H, W, N)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    _lib.check(lib.cspn2d_forward_prenorm_f32(wb.data_ptr(), hd.data_ptr(), sd.data_ptr() if sd is not None else None, out2.data_ptr(),
                                              B, H, W, N, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream), "cspn2d_forward_prenorm_f32")
    assert torch.equal(torch.nan_to_num(out2), torch.nan_to_num(pre))


def test_prenorm_is_a_2d_contract():
    """(the 2D backward takes it since round 6: tests/test_backward.py)"""
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.cspn3d_forward(torch.rand(1, 26, 4, 8, 8, device=DEV), torch.rand(1, 1, 4, 8, 8, device=DEV), None, 2, "prenorm")



def test_asm_plan_table_matches_python_planner():
    """the descriptor tables the workgroups build for themselves (same device functions, dumped by the hook library) ==
    tools/tswgen/plan.py (which the CPU emulator tests run on): the forward passes' linear plan and the band groups of the
    history / adjoint variants"""
    import ctypes
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools.tswgen.plan import build_plan, build_plan_linear
    hooks = _lib.load_hooks()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for B, H, W in ((3, 33, 304), (2, 100, 1216), (1, 7, 256), (16, 304, 1216), (64, 304, 1216), (16, 228, 304), (5, 77, 772)):
        for hist in (0, 1):
            info = _plan_info(B, H, W, 0, hist)
            if info["kind"] == 1:
                lp, hdr_ref, tab_ref = build_plan_linear(B, H, W, 24, ncu)
                assert (lp.n_wg, lp.kimg, lp.per_xcd if lp.per_xcd else 0) == (info["n_wg"], info["kimg"], info["per_xcd"] if info["xcd"] else 0)
            else:
                code = info["per_xcd"]
                xcd = (code & 0xff, (code >> 8) & 0xff, code >> 16) if info["xcd"] else None
                hdr_ref, tab_ref = build_plan(B, H, W, 24, info["n_wg"], xcd)
            assert tab_ref.shape[1] == info["stride"], (B, H, W, hist, tab_ref.shape, info)
            hdr_d = torch.zeros(info["n_wg"] * 4, dtype=torch.int32, device=DEV)
            tab_d = torch.zeros(tab_ref.size, dtype=torch.int32, device=DEV)
            assert hooks.cspn_debug_tsw_dump_plan(B, H, W, 0, hist, ctypes.c_void_p(hdr_d.data_ptr()), ctypes.c_void_p(tab_d.data_ptr()), None) == 0
            torch.cuda.synchronize()
            hdr = hdr_d.cpu().numpy().reshape(-1, 4)
            tab = tab_d.cpu().numpy().view(np.uint32).reshape(tab_ref.shape)
            assert np.array_equal(hdr[:, :3], hdr_ref[:, :3]), (B, H, W, hist)
            assert np.array_equal(tab, tab_ref), (B, H, W, hist)


def test_asm_loop_many_rows_per_group_matches_compiled_kernel():
    """so many image rows that a group's descriptor table would overflow its LDS budget: the planner must add groups
    (more workgroups than CUs); checked against the compiler-generated kernel, which plans independently"""
    B, H, W = 12000, 64, 256
    gen = torch.Generator(device=DEV).manual_seed(77)
    g = torch.randn(B, 8, H, W, generator=gen, device=DEV)
    h = torch.rand(B, 1, H, W, generator=gen, device=DEV) * 10
    a = cspn_amd.cspn2d_forward(g, h, None, 24, "8sum", "fused")
    b = cspn_amd.cspn2d_forward(g, h, None, 24, "8sum", "fused_cxx")
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert float((a - b).abs().max() / b.abs().max()) <= 1e-5
    info = _plan_info(B, H, W)
    assert info["kind"] == 0 and info["n_wg"] > 256 and info["stride"] <= 3072, info   # more pieces than a linear plan holds: band groups


def test_asm_paths_are_deterministic():
    """an LDS race or a missing wait in the generated loop would show up as run-to-run flicker (tools/stress_asm.py, short)"""
    B, H, W = 8, 304, 1216
    gen = torch.Generator(device=DEV).manual_seed(99)
    g = torch.randn(B, 8, H, W, generator=gen, device=DEV)
    h = torch.rand(B, 1, H, W, generator=gen, device=DEV) * 80
    s = (torch.rand(B, 1, H, W, generator=gen, device=DEV) < 0.01).float() * (h + 0.1)
    go = torch.randn(B, 1, H, W, generator=gen, device=DEV)
    ref = cspn_amd.cspn2d_forward(g, h, s, 24, "8sum", "fused")
    short = {n: cspn_amd.cspn2d_forward(g, h, s, n, "8sum", "fused") for n in (5, 14, 23, 31)}   # round 5: the short first pass (+ a full pass)
    gg0, gh0 = cspn_amd.cspn2d_backward(g, h, s, go, 24, "8sum")
    for i in range(12):
        assert torch.equal(cspn_amd.cspn2d_forward(g, h, s, 24, "8sum", "fused"), ref)
        for n, r in short.items():
            assert torch.equal(cspn_amd.cspn2d_forward(g, h, s, n, "8sum", "fused"), r), n
        if i % 4 == 0:
            gg, gh = cspn_amd.cspn2d_backward(g, h, s, go, 24, "8sum")
            assert torch.equal(gg, gg0) and torch.equal(gh, gh0)


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,H,W,N,norm,sp", [(1, 8, 8, 64, 3, "8sum_abs", False),      # one tile
                                               (2, 20, 30, 200, 12, "8sum", True),       # several tiles and chunks, signed gates, mask
                                               (1, 9, 17, 72, 5, "none", True),          # partial tiles, Paddle gates + mask
                                               (1, 32, 160, 304, 6, "8sum_abs", True)])  # half of config 5's volume
def test_3d_folded_modes_fused_vs_stepwise_and_oracle(B, D, H, W, N, norm, sp):
    """the normalising / masked 3D modes: fold once, then all steps in the persistent kernel (folded planes in registers, the
    constant term in LDS) -- bit-identical to fold + one launch per step, and equal to the oracle where it finishes in time"""
    gen = torch.Generator(device="cuda").manual_seed(D * 10 + N)
    g = torch.randn(B, 26, D, H, W, generator=gen, device="cuda") if norm == "8sum" else torch.rand(B, 26, D, H, W, generator=gen, device="cuda")
    if norm == "none":
        g = g / g.sum(1, keepdim=True)
    h = torch.rand(B, 1, D, H, W, generator=gen, device="cuda")
    s = (torch.rand(B, 1, D, H, W, generator=gen, device="cuda") < 0.05).float() * (h + 0.1) if sp else None
    a, ws = cspn_amd.cspn3d_forward(g, h, s, N, norm, algo="persistent", _return_ws=True)
    b = cspn_amd.cspn3d_forward(g, h, s, N, norm, algo="stepwise")
    assert torch.equal(a, b)
    assert torch.equal(a, cspn_amd.cspn3d_forward(g, h, s, N, norm))   # auto takes the fused path
    if s is not None:
        m = s != 0
        assert torch.equal(a[m], h[m])   # pinned voxels keep their input value
    if B * D * H * W <= 300000:
        assert_close(a.cpu().numpy(), cspn3d_oracle(g.cpu(), h.cpu(), None if s is None else s.cpu(), N, norm), "3d folded fused")


@pytest.mark.gpu
def test_3d_persistent_kernels_on_two_streams_do_not_starve_each_other():
    """two persistent forwards submitted to two streams at once: each needs all its workgroups resident, so they must not be
    interleaved on the device (cooperative launch); both results are the per-step kernel's, and no poll timed out"""
    B, D, H, W, N = 2, 32, 160, 304, 6
    gen = torch.Generator(device="cuda").manual_seed(17)
    g = torch.rand(B, 26, D, H, W, generator=gen, device="cuda"); g /= g.sum(1, keepdim=True)
    h1 = torch.rand(B, 1, D, H, W, generator=gen, device="cuda")
    h2 = torch.rand(B, 1, D, H, W, generator=gen, device="cuda")
    r1 = cspn_amd.cspn3d_forward(g, h1, None, N, "none", algo="stepwise")
    r2 = cspn_amd.cspn3d_forward(g, h2, None, N, "none", algo="stepwise")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(5):
        with torch.cuda.stream(s1):
            o1, w1 = cspn_amd.cspn3d_forward(g, h1, None, N, "none", algo="persistent", _return_ws=True)
        with torch.cuda.stream(s2):
            o2, w2 = cspn_amd.cspn3d_forward(g, h2, None, N, "none", algo="persistent", _return_ws=True)
        torch.cuda.synchronize()
        assert torch.equal(o1, r1) and torch.equal(o2, r2)
        lib = cspn_amd.load()
        assert _lib.load_hooks().cspn_debug_3d_persistent_error(w1.data_ptr(), B, D, H, W) == 0
        assert _lib.load_hooks().cspn_debug_3d_persistent_error(w2.data_ptr(), B, D, H, W) == 0


@pytest.mark.gpu
def test_forward_paths_can_be_captured_in_a_graph():
    """serving loops replay the propagation from a HIP graph: the 2D ring kernel and the 3D persistent kernel (plain launch while
    the stream is capturing) are captured and replayed with new input values, results equal to the eager calls"""
    gen = torch.Generator(device="cuda").manual_seed(23)
    g = torch.randn(2, 8, 96, 512, generator=gen, device="cuda")
    h = torch.rand(2, 1, 96, 512, generator=gen, device="cuda") * 10
    g3 = torch.rand(1, 26, 16, 24, 128, generator=gen, device="cuda"); g3 /= g3.sum(1, keepdim=True)
    h3 = torch.rand(1, 1, 16, 24, 128, generator=gen, device="cuda")
    cspn_amd.cspn2d_forward(g, h, None, 24, "8sum"); cspn_amd.cspn3d_forward(g3, h3, None, 6, "none")   # warm the allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gw, hw = g[..., :510].contiguous(), h[..., :510].contiguous()   # W % 4 != 0: the padded path (five launches)
    cspn_amd.cspn2d_forward(g, h, None, 31, "8sum"); cspn_amd.cspn2d_forward(gw, hw, None, 24, "8sum")
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        o2 = cspn_amd.cspn2d_forward(g, h, None, 24, "8sum")
        o2s = cspn_amd.cspn2d_forward(g, h, None, 31, "8sum")        # round 5: a short first pass of 7 iterations + a full pass
        o2w = cspn_amd.cspn2d_forward(gw, hw, None, 24, "8sum")
        o3 = cspn_amd.cspn3d_forward(g3, h3, None, 6, "none", algo="persistent")
    for seed in (1, 2):
        gen2 = torch.Generator(device="cuda").manual_seed(seed)
        h.copy_(torch.rand(2, 1, 96, 512, generator=gen2, device="cuda") * 10)
        hw.copy_(h[..., :510])
        h3.copy_(torch.rand(1, 1, 16, 24, 128, generator=gen2, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o2, cspn_amd.cspn2d_forward(g, h, None, 24, "8sum"))
        assert torch.equal(o2s, cspn_amd.cspn2d_forward(g, h, None, 31, "8sum"))
        assert torch.equal(o2w, cspn_amd.cspn2d_forward(gw, hw, None, 24, "8sum"))
        assert torch.equal(o3, cspn_amd.cspn3d_forward(g3, h3, None, 6, "none", algo="stepwise"))


@pytest.mark.gpu
def test_first_persistent_launch_of_a_process_can_be_captured():
    """round-3 advisor finding: the first persistent 3D launch on a device used to copy the status pointer into a __device__ symbol
    (a blocking copy on the null stream: it invalidates a capture).  The pointer is a kernel argument now, so a process whose FIRST
    persistent launch happens inside a graph capture works -- checked in a fresh process (this one has launched the kernel already)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import torch, cspn_amd
gen = torch.Generator(device="cuda").manual_seed(5)
g3 = torch.rand(1, 26, 16, 24, 128, generator=gen, device="cuda"); g3 /= g3.sum(1, keepdim=True)
h3 = torch.rand(1, 1, 16, 24, 128, generator=gen, device="cuda")
# one call of ANOTHER kernel of the library first: the HIP runtime loads a library's code object at its first launch, which is not
# capturable for any library; what is under test is the persistent launch's own first-time host work (its status word)
cspn_amd.cspn3d_forward(g3, h3, None, 6, "none", algo="stepwise")
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    o3 = cspn_amd.cspn3d_forward(g3, h3, None, 6, "none", algo="persistent")   # the process's first launch of the kernel
graph.replay(); torch.cuda.synchronize()
ref = cspn_amd.cspn3d_forward(g3, h3, None, 6, "none", algo="stepwise")
cspn_amd.cspn3d_check_status()
assert torch.equal(o3, ref), float((o3 - ref).abs().max())
print("CAPTURE_OK")
'''
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, PYTHONPATH=root), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "CAPTURE_OK" in r.stdout, r.stderr[-3000:]


@pytest.mark.gpu
def test_host_threads_call_the_library_concurrently():
    """the boundary promises re-entrancy (nn.DataParallel calls replicas from several Python threads, reference cspn_pytorch/eval.py:117):
    four host threads, each on its own stream, run the 2D forward (different shapes: each thread has its own plan cache), the 3D
    persistent kernel (launches chained across threads) and the error path at the same time; every result equals the serial one"""
    import threading
    shapes = [(3, 120, 516), (2, 304, 1216), (5, 77, 304), (1, 60, 772)]
    gen = torch.Generator(device=DEV).manual_seed(404)
    ins = [(torch.randn(B, 8, H, W, generator=gen, device=DEV), torch.rand(B, 1, H, W, generator=gen, device=DEV) * 80) for B, H, W in shapes]
    g3 = torch.rand(1, 26, 16, 24, 128, generator=gen, device=DEV)
    g3 /= g3.sum(1, keepdim=True)
    h3 = torch.rand(1, 1, 16, 24, 128, generator=gen, device=DEV)
    ref2 = [cspn_amd.cspn2d_forward(g, h, None, 24, "8sum") for g, h in ins]
    ref3 = cspn_amd.cspn3d_forward(g3, h3, None, 6, "none", algo="persistent")
    torch.cuda.synchronize()
    errors, lib = [], cspn_amd.load()

    def work(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for rep in range(6):
                    g, h = ins[(i + rep) % len(ins)]
                    o2 = cspn_amd.cspn2d_forward(g, h, None, 24, "8sum")
                    o3 = cspn_amd.cspn3d_forward(g3, h3, None, 6, "none", algo="persistent")
                    rc = lib.cspn2d_forward_f32(None, None, None, None, 1, 4, 4, 3, 0, None, 0, None)   # thread-local error message
                    assert rc == -1 and b"null" in lib.cspn_last_error()
                    st.synchronize()
                    assert torch.equal(o2, ref2[(i + rep) % len(ins)]) and torch.equal(o3, ref3)
        except BaseException as ex:   # noqa: BLE001 -- reported to the main thread
            errors.append("thread %d: %r" % (i, ex))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    cspn_amd.cspn3d_check_status()
    assert not errors, errors
