"""bench.py's own launcher (VERDICT r01 "What's missing" #1): `python bench.py --gpus N` with no
external torchrun must start N ranks itself, rendezvous on 127.0.0.1, and print exactly one JSON
line from rank 0.  Exercised here without a GPU through NP_BENCH_DRYRUN=1 (gloo, no kernels: the
line says "dry_run": true and carries no throughput)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def run_bench(args, extra_env=None, timeout=240):
    env = dict(os.environ, NP_BENCH_DRYRUN="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.parametrize("n", [2, 3])
def test_self_launch_prints_one_json_line(n):
    p = run_bench(["--gpus", str(n), "--steps", "4", "--warmup", "1", "--full"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    j = json.loads(lines[0])
    assert j["dry_run"] is True and j["n_gpus"] == n and j["steps"] == 4 and j["warmup"] == 1
    assert j["ranks_seen"] == n          # every spawned rank took part in the max-over-ranks collective
    assert "gloo" in j["collective"]     # ... and the line says through what (on a node: the RCCL version)
    # config 5's N > 1 report — the same function, legs and collectives a node runs, on gloo with torch.bmm for the GEMM
    c5 = j["extras"]["config5_batched_matmul_allgather"]
    legs = {"compute_only", "gathered", "overlapped_2", "overlapped_4", "overlapped_8"}          # 8 matrices per rank
    assert set(c5["ms_per_step"]) == legs == set(c5["ms_per_step_min"])
    assert all(v > 0 for v in c5["ms_per_step"].values()) and set(c5["parity_max_norm_err_vs_fp64"]) == legs - {"compute_only"}
    assert c5["parity_ok"] is True and c5["scaling"] == "strong" and "%d slab(s) of 8" % n in c5["workload"]


def test_a_plain_run_carries_only_the_headline():
    """Without --full the line holds the timed steps alone: no config-5 legs, no other configurations."""
    p = run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1"])
    assert p.returncode == 0, p.stderr[-2000:]
    j = json.loads(p.stdout.strip())
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["ranks_seen"] == 2
    assert "extras" not in j


def test_a_leg_that_fails_parity_does_not_cost_the_other_legs_their_numbers():
    """VERDICT r05 next #6a: `bench.py --gpus N --full` prints ranks_seen, the collective library and per-leg medians EVEN IF one leg's
    result is wrong — the line says parity_ok false with that leg's error, and every leg keeps its timing."""
    p = run_bench(["--gpus", "2", "--steps", "4", "--warmup", "1", "--full"], {"NP_BENCH_DRYRUN_BAD_LEG": "overlapped_2"})
    assert p.returncode == 0, p.stderr[-2000:]
    j = json.loads(p.stdout.strip())
    c5 = j["extras"]["config5_batched_matmul_allgather"]
    assert j["ranks_seen"] == 2 and c5["parity_ok"] is False
    err = c5["parity_max_norm_err_vs_fp64"]
    assert err["overlapped_2"] > 1e-3 and all(v <= 1e-6 for k, v in err.items() if k != "overlapped_2")
    assert set(c5["ms_per_step"]) == {"compute_only", "gathered", "overlapped_2", "overlapped_4", "overlapped_8"}
    assert all(v > 0 for v in c5["ms_per_step"].values())


def test_external_launcher_env_is_respected():
    """With RANK set (torch.distributed.run's convention) bench.py must NOT spawn: it is one rank."""
    p = run_bench(["--gpus", "1", "--steps", "2", "--warmup", "0"],
                  {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "NP_BENCH_FORCE_DIST": "1",
                   "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29617"})
    assert p.returncode == 0, p.stderr[-2000:]
    j = json.loads(p.stdout.strip())
    assert j["ranks_seen"] == 1


def test_world_size_mismatch_is_an_error():
    p = run_bench(["--gpus", "2", "--steps", "2", "--warmup", "0"],
                  {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "4", "MASTER_ADDR": "127.0.0.1",
                   "MASTER_PORT": "29618"})
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr


def test_dead_rank_takes_the_job_down_quickly():
    """A rank that exits non-zero must end the job (no sitting in the rendezvous time-out)."""
    p = run_bench(["--gpus", "2", "--steps", "2", "--warmup", "0"], {"NP_BENCH_DRYRUN_FAIL_RANK": "1"}, timeout=90)
    assert p.returncode != 0
    assert "rank 1 failed" in p.stderr


# ---- the config-5 report: interleaved legs, medians, nothing clamped ----

def _bench_module():
    import importlib.util
    old = os.environ.get("NP_BENCH_DRYRUN")
    os.environ["NP_BENCH_DRYRUN"] = "1"          # read once at import: no device is touched by this copy of the module
    try:
        spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["NP_BENCH_DRYRUN"]
        else:
            os.environ["NP_BENCH_DRYRUN"] = old
    return mod


class _FakeDist:
    def __init__(self, n):
        self.n, self.rank = n, 0

    def barrier_sync(self):
        pass

    def max_over_ranks(self, x):
        return x


def test_interleaved_legs_rotate_the_order_and_report_median_and_min():
    bench = _bench_module()
    calls = []
    legs = {name: (lambda name=name: calls.append(name)) for name in ("a", "b", "c")}
    out = bench.interleaved_legs(_FakeDist(1), legs, steps=2, rounds=4)
    per_round = [calls[i:i + 9] for i in range(0, len(calls), 9)]           # 3 legs x (1 warm-up + 2 timed calls)
    assert [r[0] for r in per_round] == ["a", "b", "c", "a"]                # the leg that goes first rotates
    assert all(sorted(set(r)) == ["a", "b", "c"] for r in per_round)
    for v in out.values():
        assert len(v["samples"]) == 4 and v["min"] <= v["median"] <= max(v["samples"])


def test_config5_report_never_clamps_an_inconsistent_measurement():
    bench = _bench_module()

    def legs(compute, gathered, overlapped):
        return {k: {"median": v, "min": v * 0.99, "samples": [v] * 5}
                for k, v in (("compute_only", compute), ("gathered", gathered), ("overlapped_4", overlapped))}

    slab = 64 * 1024 * 1024 * 4
    parity = {"gathered": 1e-7, "overlapped_4": 2e-7}
    good = bench._config5_report(_FakeDist(8), 64, 1024, legs(1.0e-3, 2.9e-3, 2.0e-3), slab, parity, "test", 5)
    assert good["consistent"] and good["best_gathered_form"] == "overlapped_4" and good["parity_ok"]
    assert abs(good["xgmi"]["gather_alone_ms"] - 1.9) < 1e-9
    assert abs(good["xgmi"]["link_GBps_gather_alone"] - slab / 1.9e-3 / 1e9) < 1e-6
    # computing AND gathering measured faster than computing: no "gather alone", no absurd link rate — flagged instead
    bad = bench._config5_report(_FakeDist(8), 64, 1024, legs(1.0e-3, 0.9e-3, 0.95e-3), slab, parity, "test", 5)
    assert bad["consistent"] is False and bad["inconsistent_legs"] == ["gathered", "overlapped_4"]
    assert bad["xgmi"]["gather_alone_ms"] is None and bad["xgmi"]["link_GBps_gather_alone"] is None
    assert bad["xgmi"]["inconsistent"] is True
    # within the 2 % noise band is not an inconsistency
    near = bench._config5_report(_FakeDist(1), 64, 1024, legs(1.0e-3, 0.995e-3, 1.004e-3), slab, parity, "test", 5)
    assert near["consistent"] and "xgmi" not in near
    assert bench._config5_report(_FakeDist(1), 64, 1024, legs(1e-3, 1e-3, 1e-3), slab, {"gathered": 1e-3}, "t", 5)["parity_ok"] is False
