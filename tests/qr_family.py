"""Inputs, the fp32 emulator and the metrics of the Householder QR's tests (tests/test_gpu_qr.py, tests/test_qr_reference_cpu.py).

Inputs
  exact_family   A = S P [R0; 0]: R0 upper triangular with small integer entries and a diagonal of +-d 2^e (d in {1, 2, 3}, e in
                 [-3, 3]), P a row permutation, S a diagonal of +-1, and no -0.0 anywhere.  Every reflector of the factorization is
                 an exchange of two rows (tau = 1) or the identity (tau = 0): Q has entries 0 / +-1, Q^T Q == I, Q R == A and
                 |R| == |R0| exactly, and LAPACK's sgeqrf / sorgqr give the same bits.  pow2_diag: d = 1, so that a
                 back-substitution divides by powers of two only.
  exact_rhs      for the pow2_diag family: integer x0 in [-4, 4] and b = A x0 plus small integers on A's zero rows (a residual
                 orthogonal to A's range): least squares returns x0 bit for bit.
  gaussian / graded / rank_deficient   the seeded inputs of the bound tests.

qr_emulated is the calibration of the bound tests: blocked compact-WY Householder in fp32 with panels of 64 columns, LAPACK's
slarfg rule (sign(+-0) = +), T built column by column, trailing update A2 -= V (T^T (V^T A2)), every product rounded to fp32;
the column norm and the v . x inner products of the panel in fp64 rounded once, like the device kernel.  It is independent of
the device code (numpy only); tests/test_qr_reference_cpu.py validates it against LAPACK's single-precision QR.

Metrics (float64 arithmetic on the fp32 results)
  res     ||A - Q R||_F / ||A||_F
  orth    ||Q^T Q - I||_F
  colres  max_j ||(A - Q R)[:, j]|| / ||A[:, j]||
  xerr    ||x - x64||_F / ||x64||_F against a float64 least-squares solve

RECORDED_GROWTH: the emulator's largest res / (sqrt(n) eps) and orth / (sqrt(n) eps) on Gaussian matrices of 1024 x 512 and 2048 x 256,
as profiles/linalg/qr_accuracy.log records them (`python -m tests.qr_family` prints that log).  The GPU test bounds the sizes the
emulator is too slow for by 4 x RECORDED_GROWTH x sqrt(n) eps."""
import numpy as np

EPS = 2.0 ** -23
NB = 64
f32, f64 = np.float32, np.float64

EXACT_SHAPES = [(1, 1), (2, 1), (7, 1), (5, 3), (63, 63), (64, 64), (65, 64), (65, 65), (129, 65), (200, 130), (513, 257),
                (1025, 1024), (4097, 33), (8192, 64)]
RECORDED_SHAPES = [(1024, 512), (2048, 256)]
RECORDED_GROWTH = {"res": 0.20, "orth": 2.90}     # profiles/linalg/qr_accuracy.log


def exact_family(m, n, seed=0, pow2_diag=False):
    """-> A (m x n fp32, no -0.0), R0 (n x n)"""
    rng = np.random.default_rng(7100 + 131 * m + 17 * n + seed)
    r0 = np.triu(rng.integers(-3, 4, (n, n)).astype(f64), 1)
    d = np.ones(n) if pow2_diag else rng.integers(1, 4, n).astype(f64)
    r0[np.arange(n), np.arange(n)] = np.ldexp(d, rng.integers(-3, 4, n)) * rng.choice([-1.0, 1.0], n)
    full = np.zeros((m, n))
    full[:n] = r0
    a = rng.choice([-1.0, 1.0], m)[:, None] * full[rng.permutation(m)]
    a = a.astype(f32) + f32(0.0)
    assert not np.signbit(a[a == 0]).any()
    return a, r0.astype(f32)


def exact_rhs(a, nrhs, seed=0):
    """-> b (m x nrhs fp32, exact), x0 (n x nrhs fp32)"""
    m, n = a.shape
    rng = np.random.default_rng(7300 + 131 * m + 17 * n + nrhs + seed)
    x0 = rng.integers(-4, 5, (n, nrhs)).astype(f64)
    b64 = a.astype(f64) @ x0
    zero_rows = ~a.any(axis=1)
    b64[zero_rows] += rng.integers(-5, 6, (int(zero_rows.sum()), nrhs))
    b = b64.astype(f32) + f32(0.0)
    assert np.array_equal(b.astype(f64), b64)
    return b, x0.astype(f32)


def gaussian(m, n, seed=0):
    return np.random.default_rng(7500 + 131 * m + 17 * n + seed).standard_normal((m, n)).astype(f32)


def graded(m, n):
    """column j of a Gaussian matrix times 2^((7 j mod 41) - 20): judged column by column (colres)"""
    return (gaussian(m, n, 1).astype(f64) * np.ldexp(1.0, (7 * np.arange(n)) % 41 - 20)).astype(f32)


def rank_deficient(m, n):
    """a product of m x r and r x n Gaussian factors, r = max(n // 2, 1): rank r up to rounding"""
    r = max(n // 2, 1)
    return (gaussian(m, r, 2).astype(f64) @ gaussian(r, n, 3).astype(f64)).astype(f32)


# ---- the fp32 emulator of the blocked algorithm ----

def _unit_lower(panel, w):
    v = np.tril(panel[:, :w], -1)
    v[np.arange(w), np.arange(w)] = f32(1.0)
    return v


def geqrf_emulated(a, nb=NB):
    """-> packed factor (R on and above the diagonal, v_j below), tau, the list of (j0, w, T)"""
    a = np.array(a, f32)
    m, n = a.shape
    tau = np.zeros(n, f32)
    blocks = []
    with np.errstate(all="ignore"):
        for j0 in range(0, n, nb):
            w = min(nb, n - j0)
            p = a[j0:, j0:j0 + w]
            t_mat = np.zeros((w, w), f32)
            for j in range(w):
                x, alpha = p[j + 1:, j], p[j, j]
                x64 = x.astype(f64)
                ssq = float(x64 @ x64)
                if ssq == 0.0:
                    continue                                            # tau = 0, H = I, R_jj = alpha
                nrm = f32(np.sqrt(float(alpha) * float(alpha) + ssq))
                beta = nrm if alpha < 0 else -nrm                       # sign(+-0) = +
                t = f32(f32(beta - alpha) / beta)
                v = x / f32(alpha - beta)
                z = (p[j, :].astype(f64) + v.astype(f64) @ p[j + 1:, :].astype(f64)).astype(f32)   # fp64, rounded once
                t_mat[:j, j] = -t * (t_mat[:j, :j] @ z[:j])
                t_mat[j, j] = t
                tz = t * z[j + 1:]
                p[j, j + 1:] -= tz
                p[j + 1:, j + 1:] -= np.outer(v, tz)
                p[j + 1:, j] = v
                p[j, j] = beta
                tau[j0 + j] = t
            blocks.append((j0, w, t_mat))
            if j0 + w < n:
                v = _unit_lower(p, w)
                a2 = a[j0:, j0 + w:]
                a2 -= v @ (t_mat.T @ (v.T @ a2))
    return a, tau, blocks


def qr_emulated(a, nb=NB):
    """-> Q (m x n), R (n x n, strict lower triangle +0.0f)"""
    m, n = a.shape
    packed, _, blocks = geqrf_emulated(a, nb)
    q = np.eye(m, n, dtype=f32)
    with np.errstate(all="ignore"):
        for j0, w, t_mat in reversed(blocks):
            v = _unit_lower(packed[j0:, j0:j0 + w], w)
            c = q[j0:, j0:]
            c -= v @ (t_mat @ (v.T @ c))
    return q, np.triu(packed[:n])


def lstsq_emulated(a, b, nb=NB):
    """-> x (n x nrhs), info (0, or j + 1 for the first zero on R's diagonal; then x is None)"""
    m, n = a.shape
    packed, _, blocks = geqrf_emulated(a, nb)
    zero = np.flatnonzero(np.diag(packed[:n]) == 0)
    if zero.size:
        return None, int(zero[0]) + 1
    c = np.array(b, f32)
    with np.errstate(all="ignore"):
        for j0, w, t_mat in blocks:
            v = _unit_lower(packed[j0:, j0:j0 + w], w)
            cj = c[j0:]
            cj -= v @ (t_mat.T @ (v.T @ cj))
        x = c[:n].copy()
        for i in range(n - 1, -1, -1):
            x[i] = (x[i] - packed[i, i + 1:n] @ x[i + 1:]) / packed[i, i]
    return x, 0


# ---- metrics ----

def metrics(a, q, r):
    a64, q64, r64 = a.astype(f64), q.astype(f64), r.astype(f64)
    with np.errstate(all="ignore"):
        e = a64 - q64 @ r64
        na = np.linalg.norm(a64)
        cn = np.linalg.norm(a64, axis=0)
        col = np.linalg.norm(e, axis=0) / np.where(cn == 0, 1.0, cn)
        return {"res": float(np.linalg.norm(e) / (na if na else 1.0)),
                "orth": float(np.linalg.norm(q64.T @ q64 - np.eye(q.shape[1]))),
                "colres": float(col.max())}


def xerr(a, b, x):
    x64 = np.linalg.lstsq(a.astype(f64), b.astype(f64), rcond=None)[0]
    return float(np.linalg.norm(x.astype(f64) - x64) / np.linalg.norm(x64))


def growth(a, q, r):
    """res and orth in units of sqrt(n) eps"""
    got = metrics(a, q, r)
    unit = np.sqrt(a.shape[1]) * EPS
    return {"res": got["res"] / unit, "orth": got["orth"] / unit}


def accuracy_log():
    """the text of profiles/linalg/qr_accuracy.log"""
    lines = ["# fp32 emulator of the blocked Householder QR (tests/qr_family.py: qr_emulated) on Gaussian matrices, float64 metrics,",
             "# in units of sqrt(n) eps, eps = 2^-23; numpy.linalg.qr (float64 arithmetic rounded to fp32: not an fp32 baseline) beside it",
             "# shape          res/(sqrt(n) eps)  orth/(sqrt(n) eps)   numpy: res  orth"]
    worst = {"res": 0.0, "orth": 0.0}
    for m, n in RECORDED_SHAPES:
        a = gaussian(m, n)
        g = growth(a, *qr_emulated(a))
        h = growth(a, *[x.astype(f32) for x in np.linalg.qr(a)])
        worst = {k: max(worst[k], g[k]) for k in worst}
        lines.append("%5d x %-5d    %8.3f           %8.3f             %8.3f  %8.3f" % (m, n, g["res"], g["orth"], h["res"], h["orth"]))
    lines.append("# largest: res %.3f, orth %.3f -> RECORDED_GROWTH (rounded up); the GPU bound for larger sizes is 4 x that x sqrt(n) eps"
                 % (worst["res"], worst["orth"]))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    print(accuracy_log(), end="")
