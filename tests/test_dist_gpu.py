"""Two ranks on the one GPU of the test box (gloo for the control plane, both ranks on cuda:0): the engine under
torch.distributed exactly as bench.py --gpus N drives it -- per-image-seeded batch, shard_batch, one
forward per rank, gather -- equals the single-rank result; and bench.py's own rank plumbing runs under
torch.distributed.run.  RCCL needs one device per rank, so on an 8-GPU node the same code runs with backend "nccl".

"Equals": to float-reordering noise (<= 2e-6 of the largest depth, observed ~3e-7), not bit for bit -- in the fused ring
the order in which a row's nine terms are summed depends on the ring slot the row lands in (slot 0 adds its own taps
before the taps of the row above, slots 1-3 after), and the slot is a function of the row's position in the workgroup's
stream, i.e. of the batch size.  For a FIXED shape the result is bit-reproducible (test_asm_paths_are_deterministic), and
the one-launch-per-iteration path, whose summation order is position independent, is compared bit for bit here."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, B, H, W, sparse, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        sys.path.insert(0, ROOT)
        import cspn_amd
        from cspn_amd import dist as cd
        from helpers import config_inputs
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        g, h, s = config_inputs(B, H, W, 80.0, sparse)             # the whole global batch, identical on every rank
        gs, hs, ss = cd.shard_batch([g, h, s], rank, world)
        args = (gs.cuda(), hs.cuda(), None if ss is None else ss.cuda(), 24, "8sum")
        out = cspn_amd.cspn2d_forward(*args)
        out_sw = cspn_amd.cspn2d_forward(*args, algo="stepwise")
        torch.cuda.synchronize()
        full = cd.gather_outputs(out.cpu())                        # gloo: host tensors
        full_sw = cd.gather_outputs(out_sw.cpu())
        same = None
        if rank == 0:
            args = (g.cuda(), h.cuda(), None if s is None else s.cuda(), 24, "8sum")
            single = cspn_amd.cspn2d_forward(*args).cpu()
            single_sw = cspn_amd.cspn2d_forward(*args, algo="stepwise").cpu()
            torch.cuda.synchronize()
            scale = float(single.abs().max())
            same = (bool(torch.equal(single_sw, full_sw)),                              # position-independent path: bit for bit
                    float((single - full).abs().max()) / scale)                         # fused ring: reordering noise only
        q.put((rank, tuple(full.shape), same, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # surface the traceback in the parent instead of a bare exit code
        import traceback
        q.put((rank, None, None, traceback.format_exc()))
        raise


@pytest.mark.parametrize("B,H,W,sparse", [(5, 304, 1216, False), (6, 64, 256, True)])
def test_two_ranks_share_one_gpu_bit_identical(B, H, W, sparse):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, B, H, W, sparse, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(120)
    for rank, shape, same, err in res:
        assert err is None, err
        assert shape == (B, 1, H, W)
        if rank == 0:
            assert same[0] is True
            assert same[1] <= 2e-6, same
    assert all(p.exitcode == 0 for p in procs)


def test_bench_two_ranks_launch_path():
    """bench.py under torch.distributed.run with 2 ranks on this box's GPU (shared_gpu mode: gloo, no broadcast):
    the exact command line the driver uses for N > 1, at a small batch."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--batch-per-gpu", "4", "--global-batch", "6", "--prewarm-s", "0.1", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 5 and res["scaling"] == "weak"
    assert res["parity_checked"]["ok"] and res["parity_checked"]["all_ranks_ok"]
    assert res["value"] > 0 and res["roofline"]["frac"] > 0
    # round 4: what the driver's N > 1 run must show even if a collective misbehaves -- who ran where, the broadcast's fate, and
    # BASELINE config 3 as written (the strong shape) beside the weak-scaling headline
    for rank in (0, 1):
        assert "[bench.py rank %d/2] device 0 of 1" % rank in r.stderr, r.stderr[-2000:]
    assert res["backend"] == "gloo" and res["devices"]["visible"] == 1
    assert "broadcast_ms" in res and res["broadcast_ms"] is None and res["broadcast_bytes"] == 0 and "broadcast_error" not in res
    st = res["strong"]
    assert st["global_batch"] == 6 and st["B_per_gpu"] == 3 and st["value"] > 0 and 0 < st["roofline_frac_per_gpu"] < 1
    assert st["parity_checked"]["ok"] and st["parity_checked"]["all_ranks_ok"]
    assert "notes" not in res, res.get("notes")


def test_bench_two_ranks_strong_scaling_shards_the_global_batch():
    """--scaling strong (BASELINE config 3's shape: ONE global batch sharded over the ranks, the scatter of reference
    cspn_pytorch/eval.py:115-118): 7 images over 2 ranks = 4 + 3, the reported value counts every image once"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--scaling", "strong", "--global-batch", "7", "--prewarm-s", "0.1", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert res["n_gpus"] == 2 and res["scaling"] == "strong"
    assert res["config"]["global_batch"] == 7 and res["config"]["B_per_gpu"] == 4
    assert res["parity_checked"]["ok"] and res["parity_checked"]["all_ranks_ok"]
    mpix = 7 * 304 * 1216 * 24 * 5 / 1e6
    assert abs(res["value"] * res["ms_per_step"] * 5 / 1e3 - mpix) <= 1e-3 * mpix
