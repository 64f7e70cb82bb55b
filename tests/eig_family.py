"""Inputs, metrics and the CPU calibration of the symmetric eigensolver's tests (tests/test_gpu_eigh.py,
tests/test_eig_reference_cpu.py).

Inputs
  exact_diagonal  diag(d) with DISTINCT entries +-j 2^e at permuted positions, one +0.0 and one -0.0 among them from n = 3 on:
                  nothing rotates, so w = the stably sorted d bit for bit and v is a permutation matrix of 0 / +1.
  toeplitz        tridiagonal (2, -1): eigenvalues 4 sin^2(k pi / (2 (n + 1))), eigenvectors sqrt(2 / (n + 1)) sin(i k pi / (n + 1)).
  hadamard_case   H diag(d) H^T / n, Sylvester Hadamard H, d = -n/2 .. n/2 - 1: exact in fp32 and exactly symmetric (asserted).
  exchange        ones on the antidiagonal: -1 (n // 2 times) and +1; zero diagonal, repeated eigenvalues.
  rank_one_shift  3 I + u u^T: n - 1 eigenvalues equal to 3, one 3 + u.u.
  random_symmetric / indefinite / graded   the seeded inputs of the bound tests.

Metrics (float64 arithmetic on the fp32 results, eps = 2^-23, ||a||_2 from numpy's float64 eigvalsh of the fp32 input)
  res    max_j ||a v_j - w_j v_j||_2 / ||a||_2
  orth   max |V^T V - I|
  werr   max |w - w64| / ||a||_2

jacobi_eigh_emulated is the calibration of the bound tests: two-sided cyclic Jacobi, fp32 storage, fp64 rotations rounded once,
unblocked, round-robin pairs, the device code's activity rule (|w_pq| > eps max|a|) — the same algorithm class as the device
code and independent of it (no blocking, no 64 x 64 fp64 solve).  It takes 7 to 16 seconds per input around n = 512, so its metrics
on the three bound families at 512 and on the Toeplitz matrix of 500 are recorded in tests/golden/eig_emulator_recorded.json
(`python -m tests.eig_family` writes the file; emulator_metrics() and closed_form_emulator_metrics() read it) and computed on the
spot up to n = 257."""
import json
from pathlib import Path

import numpy as np

from tests.svd_family import hadamard, round_robin_steps

EPS = 2.0 ** -23
f32 = np.float32

EXACT_SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 192, 257, 1000, 2049]
TOEPLITZ_SIZES = [2, 33, 64, 65, 129, 500, 1000]
HADAMARD_SIZES = [64, 256, 1024]
EXCHANGE_SIZES = [2, 65, 128, 257]
BOUND_SIZES = [2, 7, 33, 64, 65, 100, 128, 192, 257, 512, 1000, 1024, 2048]
METRICS = ("res", "orth", "werr")


def exact_diagonal(n, seed=0):
    """-> a (diag(d), fp32), d in diagonal order"""
    rng = np.random.default_rng(5151 + 1009 * n + seed)
    pick = rng.choice(2048 * 7, size=n, replace=False)
    d = np.ldexp((2 * (pick % 2048) + 1).astype(np.float64), pick // 2048 - 3) * rng.choice([-1.0, 1.0], n)
    d = d.astype(f32)
    if n >= 3:
        d[0], d[1] = f32(0.0), f32(-0.0)
        d[2] = -abs(d[2])
    d = d[rng.permutation(n)]
    return np.diag(d), d     # np.diag leaves +0.0 off the diagonal; the diagonal keeps its bits, -0.0 included


def sorted_stable(d):
    """ascending, ties (-0.0 == +0.0 among them) in diagonal order: -> values, the order"""
    order = np.argsort(d, kind="stable")
    return d[order], order


def toeplitz(n):
    a = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    k = np.arange(1, n + 1)
    lam = 4.0 * np.sin(k * np.pi / (2.0 * (n + 1))) ** 2
    vec = np.sqrt(2.0 / (n + 1)) * np.sin(np.outer(k, k) * np.pi / (n + 1))       # column k - 1 belongs to lam[k - 1]
    return a.astype(f32), lam, vec


def hadamard_case(n):
    """-> a (fp32, exact, exactly symmetric), its spectrum ascending"""
    d = np.arange(-n // 2, n // 2, dtype=np.float64)
    H = hadamard(n)
    a64 = (H * d) @ H.T / n
    a = a64.astype(f32)
    assert np.array_equal(a.astype(np.float64), a64) and np.array_equal(a, a.T)
    return a, d


def exchange(n):
    return np.eye(n, dtype=f32)[::-1].copy(), np.concatenate((-np.ones(n // 2), np.ones(n - n // 2)))


def rank_one_shift(n):
    rng = np.random.default_rng(41000 + n)
    u = rng.integers(-3, 4, n).astype(np.float64)
    a = 3.0 * np.eye(n) + np.outer(u, u)                                          # small integers: exact in fp32
    lam = np.full(n, 3.0)
    lam[-1] = 3.0 + u @ u
    return a.astype(f32), lam


def random_symmetric(n):
    rng = np.random.default_rng(42000 + n)
    g = rng.standard_normal((n, n)).astype(f32)
    return np.tril(g) + np.tril(g, -1).T


def indefinite(n):
    """a random orthogonal similarity of a spectrum spread over [-1, 1], symmetrised exactly"""
    rng = np.random.default_rng(43000 + n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = ((q * np.linspace(-1.0, 1.0, n)) @ q.T).astype(f32)
    return np.tril(a) + np.tril(a, -1).T


def graded(n):
    """D S D with D = powers of two from 1 down to 2^-12 on rows and columns: exactly symmetric"""
    s = random_symmetric(n).astype(np.float64)
    d = np.ldexp(1.0, -(np.arange(n) * 12 // max(n - 1, 1)))
    return (s * d[:, None] * d[None, :]).astype(f32)


BOUND_FAMILIES = {"symmetric": random_symmetric, "indefinite": indefinite, "graded": graded}


def w64(a):
    return np.linalg.eigvalsh(a.astype(np.float64))


def metrics(a, w, v, lam=None):
    """-> dict(res, orth, werr) in units of 1 (divide by EPS to read them); lam: the float64 spectrum, ascending"""
    a64, w_, v_ = a.astype(np.float64), w.astype(np.float64), v.astype(np.float64)
    if lam is None:
        lam = w64(a)
    n = a.shape[0]
    na = float(np.abs(lam).max()) if n else 0.0
    if na == 0.0:
        na = 1.0
    r = a64 @ v_ - v_ * w_
    return {"res": float(np.sqrt((r * r).sum(axis=0)).max() / na), "orth": float(np.abs(v_.T @ v_ - np.eye(n)).max()),
            "werr": float(np.abs(w_ - lam).max() / na)}


def apply_sign_rule(v):
    """the component of largest magnitude in each column, the first such in index order, is positive"""
    v = v.copy()
    at = np.argmax(np.abs(v), axis=0)
    neg = v[at, np.arange(v.shape[1])] < 0
    v[:, neg] = -v[:, neg]
    return v


def jacobi_eigh_emulated(A, tol=EPS, max_sweeps=60):
    """-> w (ascending, stable), v (columns, sign rule applied), sweeps taken (the one that rotates nothing included), converged.
    Only the lower triangle of A is read."""
    A = np.asarray(A, f32)
    n = A.shape[0]
    W = np.tril(A)
    upper = np.triu_indices(n, 1)
    W[upper] = W.T[upper]                      # mirrored, not added: a -0.0 on the diagonal keeps its sign
    Vt = np.eye(n, dtype=f32)
    lim = tol * float(np.abs(W).max()) if n else 0.0
    sweeps, ok = 0, False
    for sweeps in range(1, max_sweeps + 1):
        rotated = 0
        for p, q in round_robin_steps(n):
            if p.size == 0:
                continue
            app, aqq, apq = W[p, p].astype(np.float64), W[q, q].astype(np.float64), W[q, p].astype(np.float64)
            do = np.abs(apq) > lim
            if not do.any():
                continue
            p, q, app, aqq, apq = p[do], q[do], app[do], aqq[do], apq[do]
            rotated += p.size
            z = (aqq - app) / (2.0 * apq)
            t = np.where(z >= 0, 1.0, -1.0) / (np.abs(z) + np.sqrt(1.0 + z * z))
            c64 = 1.0 / np.sqrt(1.0 + t * t)
            c, s = c64.astype(f32)[:, None], (c64 * t).astype(f32)[:, None]
            for M in (W, Vt):
                Mp, Mq = M[p], M[q]
                M[p], M[q] = c * Mp - s * Mq, s * Mp + c * Mq
            Wp, Wq = W[:, p], W[:, q]
            W[:, p], W[:, q] = c.T * Wp - s.T * Wq, s.T * Wp + c.T * Wq
            W[p, p], W[q, q] = (app - t * apq).astype(f32), (aqq + t * apq).astype(f32)
            W[p, q] = W[q, p] = f32(0.0)
        if rotated == 0:
            ok = True
            break
    w, order = sorted_stable(np.diag(W).copy())
    return w, apply_sign_rule(Vt[order].T.copy()), sweeps, ok


RECORDED = Path(__file__).resolve().parent / "golden" / "eig_emulator_recorded.json"
RECORDED_SIZE = 512
LIVE_SIZE = 257                                  # up to here the emulator runs inside the test (about a second at 257)
RECORDED_CLOSED_FORMS = {"toeplitz-500": lambda: toeplitz(500)[:2]}   # name -> (a, the closed-form spectrum)


def emulator_metrics(family, n):
    """res, orth and werr of the emulator on BOUND_FAMILIES[family](n): recorded at n = 512, computed below it"""
    if n == RECORDED_SIZE:
        return json.loads(RECORDED.read_text())[family]
    assert n < RECORDED_SIZE
    a = BOUND_FAMILIES[family](n)
    w, v, _, ok = jacobi_eigh_emulated(a)
    assert ok
    return metrics(a, w, v)


def closed_form_emulator_metrics(name, a, lam):
    """the same for a closed-form input (werr against the formula lam): computed up to LIVE_SIZE, recorded under `name-n` above"""
    n = a.shape[0]
    if n > LIVE_SIZE:
        return json.loads(RECORDED.read_text())["%s-%d" % (name, n)]
    w, v, _, ok = jacobi_eigh_emulated(a)
    assert ok
    return metrics(a, w, v, lam)


if __name__ == "__main__":
    out = {}
    cases = [(family, make(RECORDED_SIZE), None) for family, make in BOUND_FAMILIES.items()]
    cases += [(name,) + make() for name, make in RECORDED_CLOSED_FORMS.items()]
    for name, a, lam in cases:
        w, v, sweeps, ok = jacobi_eigh_emulated(a)
        assert ok
        out[name] = dict(metrics(a, w, v, lam), sweeps=sweeps)
        print(name, out[name], flush=True)
    RECORDED.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
