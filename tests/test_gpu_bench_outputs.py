"""bench.py's plain run and --dump-outputs on the GPU: the line carries the headline only, and the dump holds the same seeded
rows of every product of the last timed step — float32, at most 64 MB, C_i = C_0 * 2^-i bit for bit, C_0 within 1e-5 of fp64."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from numpower_amd import synth

ROOT = Path(__file__).resolve().parent.parent


def _bench_constants():
    spec = importlib.util.spec_from_file_location("bench_constants", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # module level only: main() is not run
    return mod


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_products(tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("NP_BENCH_") and k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    j = json.loads(lines[0])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "GFLOP/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert not {"extras", "cpu_baseline", "parity"} & set(j)

    bench = _bench_constants()
    n = 4096
    files = sorted(out.glob("*.npy"))
    assert [f.name for f in files] == ["matmul_C%d_rows.npy" % i for i in range(bench.PRODUCT_SETS)]
    assert sum(f.stat().st_size for f in files) <= 64e6
    got = [np.load(f) for f in files]
    for c in got:
        assert c.dtype == np.float32 and c.shape == (bench.DUMP_ROWS, n)
    for i, c in enumerate(got[1:], start=1):
        assert (c.view(np.uint32) == (got[0] * np.float32(2.0 ** -i)).view(np.uint32)).all(), i
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, size=bench.DUMP_ROWS, replace=False))
    A = synth.uniform((n, n), 3, -1.0, 1.0)[rows].astype(np.float64)
    B = synth.uniform((n, n), 4, -1.0, 1.0).astype(np.float64)
    err = np.abs(got[0] - A @ B) / (np.abs(A) @ np.abs(B))
    assert float(err.max()) <= 1e-5
