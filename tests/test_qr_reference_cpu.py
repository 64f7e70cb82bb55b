"""CPU-tier validation of what tests/test_gpu_qr.py compares the device QR with (tests/qr_family.py).

  - On the exact family the fp32 emulator of the blocked algorithm equals numpy.linalg.qr with == at every shape the GPU test uses
    (and scipy.linalg.qr in float32, LAPACK's sgeqrf / sorgqr, when SciPy imports); its least squares returns x0 with ==.
  - On Gaussian matrices the emulator's res and orth are within 2 x those of SciPy's float32 QR: the ratios measured were 0.78 - 1.21
    at 64 x 64, 200 x 130, 513 x 257, 1024 x 512 and 2048 x 256; the factor 2 covers another seed and another BLAS.
  - profiles/linalg/qr_accuracy.log holds the emulator's growth at 1024 x 512 and 2048 x 256, and qr_family.RECORDED_GROWTH is its
    largest row rounded up: the constant behind the GPU test's bound for its largest sizes."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import qr_family as F

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("m,n", F.EXACT_SHAPES)
def test_the_emulator_equals_lapack_on_the_exact_family(m, n):
    a, r0 = F.exact_family(m, n)
    q, r = F.qr_emulated(a)
    qn, rn = np.linalg.qr(a)
    assert qn.dtype == np.float32 and np.array_equal(q, qn) and np.array_equal(r, rn)
    assert set(np.unique(q)) <= {-1.0, 0.0, 1.0}
    q64 = q.astype(np.float64)
    assert np.array_equal(q64.T @ q64, np.eye(n)) and np.array_equal(q64 @ r.astype(np.float64), a.astype(np.float64))
    assert np.array_equal(np.abs(r), np.abs(r0))
    _, tau, blocks = F.geqrf_emulated(a)
    assert set(np.unique(tau)) <= {0.0, 1.0} and all(np.abs(t).max() <= 1.0 for _, _, t in blocks)


@pytest.mark.parametrize("m,n", F.EXACT_SHAPES)
def test_the_emulator_equals_scipy_float32_on_the_exact_family(m, n):
    sl = pytest.importorskip("scipy.linalg")
    a, _ = F.exact_family(m, n)
    q, r = F.qr_emulated(a)
    qs, rs = sl.qr(a, mode="economic")
    assert qs.dtype == np.float32 and np.array_equal(q, qs) and np.array_equal(r, rs)


@pytest.mark.parametrize("m,n", F.EXACT_SHAPES)
def test_the_emulated_least_squares_returns_x0(m, n):
    a, _ = F.exact_family(m, n, pow2_diag=True)
    for nrhs in (1, 3, 65):
        b, x0 = F.exact_rhs(a, nrhs)
        x, info = F.lstsq_emulated(a, b)
        assert info == 0 and np.array_equal(x, x0)


def test_the_emulated_info_rule():
    a, _ = F.exact_family(70, 66, pow2_diag=True)
    b, _ = F.exact_rhs(a, 2)
    for j in (0, 63, 64, 65):
        low = a.copy()
        low[:, j] = 0.0                     # column j of R0 is zero: R_jj == 0 exactly, and no earlier diagonal is
        x, info = F.lstsq_emulated(low, b)
        assert info == j + 1 and x is None


@pytest.mark.parametrize("m,n", [(64, 64), (200, 130), (513, 257), (1024, 512), (2048, 256)])
def test_the_emulator_is_as_accurate_as_lapack_in_single_precision(m, n):
    sl = pytest.importorskip("scipy.linalg")
    a = F.gaussian(m, n)
    got = F.metrics(a, *F.qr_emulated(a))
    ref = F.metrics(a, *sl.qr(a, mode="economic"))
    print("%d x %d: emulator res %.3g orth %.3g, sgeqrf res %.3g orth %.3g" % (m, n, got["res"], got["orth"], ref["res"], ref["orth"]))
    assert got["res"] <= 2 * ref["res"] and got["orth"] <= 2 * ref["orth"]


def test_the_recorded_growth_is_what_the_log_holds_and_what_the_emulator_gives():
    text = (ROOT / "profiles" / "linalg" / "qr_accuracy.log").read_text()
    rows = re.findall(r"^\s*(\d+) x (\d+)\s+([\d.]+)\s+([\d.]+)", text, flags=re.M)
    assert [(int(m), int(n)) for m, n, _, _ in rows] == F.RECORDED_SHAPES
    logged = {"res": max(float(r[2]) for r in rows), "orth": max(float(r[3]) for r in rows)}
    for key in ("res", "orth"):
        assert logged[key] <= F.RECORDED_GROWTH[key] <= 1.1 * logged[key], key
    for m, n in F.RECORDED_SHAPES:     # and the log is reproducible here: within a quarter, another BLAS sums in another order
        a = F.gaussian(m, n)
        live = F.growth(a, *F.qr_emulated(a))
        for key in ("res", "orth"):
            assert live[key] <= 1.25 * F.RECORDED_GROWTH[key], (m, n, key, live[key])
