"""Exact-arithmetic LU inputs and a float64 host reference for them (test infrastructure, numpy only).

A case is M = Q L U with Q a permutation (row perm[i] of M is row i of L U), L unit lower triangular and U upper
triangular, both dyadic, with U's diagonal a power of two (or 0 at a designed zero pivot).  When the exactness certificate
holds (`certify`), every partial sum any summation order can form is a multiple of 2^-d below 2^(24 - d), so fp32 partial
pivoting returns exactly this L, U and these pivots whatever its order of summation, FMA or MFMA tiling, and a solve with
an integer x and b = M x returns x exactly.  The expected values are then complete: tests compare element for element.

The pivot is the first row with the largest |value| (isamax): a designed row wins because every other row of its column
has |L| <= 1/2, or |L| = 1 and sits LATER in the current row order (a tie by design).  Pivots are 0-based; info is 1 + the
first zero pivot, and the factorization goes on past it without dividing (sgetf2).

L and U are held sparse (coordinates + values), so a case of n = 46341 costs O(nnz) on the host; `dense_M()` is for
n up to a few thousand.
"""
from __future__ import annotations

import numpy as np

L_VALUES = np.array([-0.5, -0.375, -0.25, -0.125, 0.125, 0.25, 0.375, 0.5])
U_VALUES = np.array([-3.0, -2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 3.0])


# ---- the host reference ----------------------------------------------------------------------------------------------

def getf2_ref(M):
    """Unblocked LU with partial pivoting in float64, LAPACK sgetf2's semantics: the first row with the largest |value|
    pivots, row exchanges apply to whole rows, info = 1 + the first exactly-zero pivot, no division by it.
    Returns (packed L\\U, ipiv 0-based int64, info)."""
    A = np.array(M, dtype=np.float64, copy=True)
    n = A.shape[0]
    ipiv = np.zeros(n, np.int64)
    info = 0
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))    # argmax: the first maximum
        ipiv[k] = p
        if p != k:
            A[[k, p]] = A[[p, k]]
        d = A[k, k]
        if d != 0.0:
            A[k + 1:, k] /= d
        elif info == 0:
            info = k + 1
        if k + 1 < n:
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return A, ipiv, info


def perm_from_ipiv(ipiv):
    """perm[r] = the row of M that the exchanges bring to row r (laswp order): P M = L U with P[r, perm[r]] = 1."""
    order = np.arange(len(ipiv), dtype=np.int64)
    for k, p in enumerate(ipiv.tolist()):
        if p != k:
            order[k], order[p] = order[p], order[k]
    return order


def det_ref(diag, ipiv, info):
    """The reference's det loop (linalg.c:286-297): U's diagonal multiplied in index order in fp32, left to right, the sign
    of the pivot parity, 0.0f when info > 0.  Returns an np.float32."""
    if info > 0:
        return np.float32(0.0)
    d = np.asarray(diag, np.float32)
    det = np.float32(1.0)
    if len(d):
        with np.errstate(over="ignore", under="ignore"):
            det = np.multiply.accumulate(np.concatenate([[np.float32(1.0)], d]), dtype=np.float32)[-1]
    swaps = int(np.count_nonzero(np.asarray(ipiv) != np.arange(len(ipiv))))
    return np.float32(-det) if swaps & 1 else np.float32(det)


# ---- the exactness certificate ---------------------------------------------------------------------------------------

def certify_stepwise(M):
    """For small matrices whose certificate is the unblocked order itself (the classic Wilkinson matrix, whose U grows
    to 2^(n-1)): every product and every value the one-step-at-a-time elimination forms is an fp32 number."""
    A = np.array(M, np.float64)
    n = A.shape[0]
    assert (A.astype(np.float32) == A).all()
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]
        if A[k, k] != 0:
            A[k + 1:, k] /= A[k, k]
        prod = np.outer(A[k + 1:, k], A[k, k + 1:])
        A[k + 1:, k + 1:] -= prod
        assert (prod.astype(np.float32) == prod).all() and (A.astype(np.float32) == A).all(), ("inexact at step", k)
    return True


def dyadic_exponent(v, limit=60):
    """The smallest d with every entry of v a multiple of 2^-d."""
    v = np.asarray(v, np.float64).ravel()
    for d in range(limit + 1):
        s = v * 2.0 ** d
        if (s == np.floor(s)).all():
            return d
    raise AssertionError("not dyadic within 2^-%d" % limit)


def _is_pow2(v):
    m, _ = np.frexp(np.abs(v))
    return m == 0.5


def _spmm(n, ar, ac, av, br, bc, bv):
    """(rows, cols, values) of A B for n x n A, B given as coordinates: duplicates summed, exact zeros dropped, in
    O(sum over A's entries of the entries in B's matching row)."""
    order = np.argsort(br, kind="stable")
    br, bc, bv = br[order], bc[order], bv[order]
    cnt = np.bincount(br, minlength=n)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rep = cnt[ac]
    keep = rep > 0
    ar, ac, av, rep = ar[keep], ac[keep], av[keep], rep[keep]
    tot = int(rep.sum())
    src = np.repeat(start[ac], rep) + np.arange(tot) - np.repeat(np.cumsum(rep) - rep, rep)
    key = np.repeat(ar, rep) * n + bc[src]
    ukey, inv = np.unique(key, return_inverse=True)
    sums = np.bincount(inv, weights=np.repeat(av, rep) * bv[src])
    nz = sums != 0.0
    ukey, sums = ukey[nz], sums[nz]
    return ukey // n, ukey % n, sums


# ---- a case ----------------------------------------------------------------------------------------------------------

class Case:
    """M = Q L U, held as coordinates.  L: strict lower part (Lr > Lc); U: upper part incl. its diagonal (Ur <= Uc), zero
    entries never listed.  diag: U's diagonal (0 at zero pivots)."""

    def __init__(self, n, ipiv, Lr, Lc, Lv, Ur, Uc, Uv, zero_pivots=()):
        self.n = int(n)
        self.ipiv = np.asarray(ipiv, np.int64)
        self.perm = perm_from_ipiv(self.ipiv)
        self.Lr, self.Lc, self.Lv = (np.asarray(x) for x in (Lr, Lc, Lv))
        self.Ur, self.Uc, self.Uv = (np.asarray(x) for x in (Ur, Uc, Uv))
        self.diag = np.zeros(self.n)
        on = self.Ur == self.Uc
        self.diag[self.Ur[on]] = self.Uv[on]
        self.zero_pivots = tuple(sorted(zero_pivots))
        self.info = self.zero_pivots[0] + 1 if self.zero_pivots else 0
        self.M = None          # M itself where the sparse product would round (the classic Wilkinson matrix)

    # expected results
    def det(self):
        """det of M (= det of M^T) as the reference computes it."""
        return det_ref(self.diag, self.ipiv, self.info)

    def packed_coords(self):
        """(rows, cols, values) of the packed L\\U, every listed value nonzero, every other entry zero."""
        return (np.concatenate([self.Lr, self.Ur]), np.concatenate([self.Lc, self.Uc]),
                np.concatenate([self.Lv, self.Uv]))

    def packed(self):
        out = np.zeros((self.n, self.n))
        r, c, v = self.packed_coords()
        out[r, c] = v
        return out

    def L(self):
        out = np.eye(self.n)
        out[self.Lr, self.Lc] = self.Lv
        return out

    def U(self):
        out = np.zeros((self.n, self.n))
        out[self.Ur, self.Uc] = self.Uv
        return out

    def P(self):
        out = np.zeros((self.n, self.n))
        out[np.arange(self.n), self.perm] = 1.0
        return out

    # the input
    def M_coords(self):
        """(rows, cols, values) of M = Q L U, duplicates summed, in O(nnz(L) * nnz per row of U)."""
        n = self.n
        if self.M is not None:
            r, c = np.nonzero(self.M)
            return r, c, self.M[r, c]
        r, c, v = _spmm(n, np.concatenate([np.arange(n), self.Lr]), np.concatenate([np.arange(n), self.Lc]),
                        np.concatenate([np.ones(n), self.Lv]), self.Ur, self.Uc, self.Uv)
        return self.perm[r], c, v

    def dense_M(self):
        out = np.zeros((self.n, self.n))
        r, c, v = self.M_coords()
        out[r, c] = v
        return out

    def matvec(self, x):
        """M x in float64, O(nnz), for x of shape (n,) or (n, k)."""
        r, c, v = self.M_coords()
        x = np.asarray(x, np.float64)
        out = np.zeros((self.n,) + x.shape[1:])
        np.add.at(out, r, v.reshape((-1,) + (1,) * (x.ndim - 1)) * x[c])
        return out

    def certify(self, x=None, x_coords=None):
        """The exactness certificate: dyadic entries, U's diagonal powers of two (0 only at the designed zero pivots),
        |L| <= 1 strictly below the diagonal and 2 max(|L| |U| |x|) < 2^(24 - d) with d = the dyadic exponents of L, U
        and x together (x dense, or x_coords = (rows, cols, values) of a sparse x).  A diagonal U (no off-diagonal entry) is exact at any scale: every value the factorization forms
        is one product L[i, k] U[k, k] — there the normal fp32 range is checked instead."""
        n = self.n
        assert (self.Lr > self.Lc).all() and (self.Ur <= self.Uc).all()
        assert (self.Lv != 0).all() and (self.Uv != 0).all()
        assert (np.abs(self.Lv) <= 1.0).all()
        zp = np.zeros(n, bool)
        zp[list(self.zero_pivots)] = True
        assert (self.diag[zp] == 0).all() and _is_pow2(self.diag[~zp]).all()
        for k in self.zero_pivots:
            assert not (self.Lc == k).any(), "a zero pivot's L column must be zero"
        if not (self.Ur != self.Uc).any() and x is None:
            prod = np.abs(self.Lv) * np.abs(self.diag[self.Lc])
            assert (prod == 0).all() or (prod[prod > 0].min() >= 2.0 ** -126 and prod.max() < 2.0 ** 127)
            return True
        if x_coords is not None:
            xa = np.zeros(n)
            np.maximum.at(xa, x_coords[0], np.abs(x_coords[2]))
            dx = dyadic_exponent(x_coords[2])
        else:
            xa = np.ones(n) if x is None else np.abs(np.asarray(x, np.float64)).reshape(n, -1).max(1)
            dx = 0 if x is None else dyadic_exponent(x)
        xa = np.maximum(xa, 1.0)
        d = dyadic_exponent(self.Lv) + dyadic_exponent(self.Uv) + dx
        w = np.bincount(self.Ur, weights=np.abs(self.Uv) * xa[self.Uc], minlength=n)
        z = w + np.bincount(self.Lr, weights=np.abs(self.Lv) * w[self.Lc], minlength=n)
        assert 2.0 * z.max() < 2.0 ** (24 - d), ("inexact", 2.0 * z.max(), d)
        return True


# ---- constructions ---------------------------------------------------------------------------------------------------

def _diag_walk(rng, n, lo=-40, hi=40):
    """Powers of two with random signs whose running product stays within 2^lo .. 2^hi (no overflow, no denormal)."""
    e = np.zeros(n, np.int64)
    run = 0
    steps = rng.integers(-1, 2, n)
    for k in range(n):
        s = int(steps[k])
        if run + s > hi or run + s < lo:
            s = -s
        e[k] = s
        run += s
    return np.ldexp(np.where(rng.random(n) < 0.5, -1.0, 1.0), e)


def _random_cols(rng, n, per, strict_lower):
    """For each column (lower) or row (upper) j, up to `per` distinct partners strictly beyond j, a uniform random subset
    of the room beyond j: the first `per` distinct values of a run of uniform draws (a set drawn afresh when the run had
    too few)."""
    out_a, out_b = [], []
    js = np.arange(n - 1)
    room = n - 1 - js
    k = np.minimum(room, per)
    for size in np.unique(k):
        sel = js[k == size]
        r = room[sel]
        picks = np.floor(rng.random((len(sel), int(size) * 3)) * r[:, None]).astype(np.int64)
        for row, (j, rr) in enumerate(zip(sel.tolist(), r.tolist())):
            if rr <= size:
                u = np.arange(rr)
            else:
                p = picks[row]
                _, first = np.unique(p, return_index=True)
                u = p[np.sort(first)][:size]        # in draw order, not sorted: no bias towards small offsets
                if len(u) < size:
                    u = rng.choice(rr, int(size), replace=False)
            out_a.append(np.full(len(u), j))
            out_b.append(j + 1 + u)
    a = np.concatenate(out_a) if out_a else np.zeros(0, np.int64)
    b = np.concatenate(out_b) if out_b else np.zeros(0, np.int64)
    return (b, a) if strict_lower else (a, b)


def generic(n, seed, per=8, swap_prob=0.75, zero_pivots=(), ties=(), parity=None, diag=None, u_offdiag=True,
            first_swap=False):
    """A random Q and dyadic L, U.

    per          nonzeros per column of L below the diagonal and per row of U right of it (at most)
    zero_pivots  steps k with U[k, k] = 0 and L[k+1:, k] = 0 (and no exchange: the designed row is already at k)
    ties         (k, delta): at step k a non-pivot row delta positions after the designed pivot row gets |L| = 1
    parity       0 / 1: force the number of exchanges even / odd
    diag         U's diagonal (default: a bounded random walk of powers of two)
    u_offdiag    False: U diagonal (with `diag` at any scale, see Case.certify).  True: besides the random partners, every
                 row of U has an entry in the last column, so that every panel's U12 reaches the last column tile
    first_swap   the first step exchanges rows (ipiv[0] > 0)
    """
    rng = np.random.default_rng(seed)
    n = int(n)
    zero_pivots = sorted(set(int(k) for k in zero_pivots))
    tie_at = {}
    for k, delta in ties:
        tie_at.setdefault(int(k), []).append(int(delta))
    ipiv = np.arange(n, dtype=np.int64)
    sw = rng.random(n) < swap_prob
    ks = np.nonzero(sw)[0]
    ipiv[ks] = ks + np.floor(rng.random(len(ks)) * (n - ks)).astype(np.int64)
    if first_swap and n > 1:
        ipiv[0] = 1 + int(rng.integers(0, n - 1))
    fixed = set(zero_pivots) | ({0} if first_swap else set())
    for k, deltas in tie_at.items():   # room for the tie rows after the designed row
        top = n - 1 - max(deltas)
        assert top >= k, ("no room for a tie", k, deltas, n)
        ipiv[k] = k + int(rng.integers(0, min(top - k, 7) + 1))
        fixed.add(k)
    for k in zero_pivots:
        ipiv[k] = k
    if parity is not None and n >= 2:
        swaps = int(np.count_nonzero(ipiv != np.arange(n)))
        if swaps % 2 != parity:
            k = max(j for j in range(n - 1) if j not in fixed)
            ipiv[k] = k + 1 if ipiv[k] == k else k
    Lr, Lc = _random_cols(rng, n, per, True)
    Lv = rng.choice(L_VALUES, len(Lr))
    if u_offdiag:
        Ur, Uc = _random_cols(rng, n, per, False)
        last = np.setdiff1d(np.arange(n - 1), Ur[Uc == n - 1])
        Ur = np.concatenate([Ur, last])
        Uc = np.concatenate([Uc, np.full(len(last), n - 1)])
        Uv = rng.choice(U_VALUES, len(Ur))
    else:
        Ur = Uc = Uv = np.zeros(0, np.int64)
    d = _diag_walk(rng, n) if diag is None else np.asarray(diag, np.float64)
    assert len(d) == n
    if zero_pivots:
        d = d.copy()
        d[zero_pivots] = 0.0
        drop = np.isin(Lc, zero_pivots)
        Lr, Lc, Lv = Lr[~drop], Lc[~drop], Lv[~drop]
    if tie_at:
        # positions at each tie step: simulate the exchanges before it
        order = np.arange(n, dtype=np.int64)            # position -> row of M
        perm = perm_from_ipiv(ipiv)
        logical = np.empty(n, np.int64)
        logical[perm] = np.arange(n)                    # row of M -> logical row (row of L U)
        add_r, add_c, add_v = [], [], []
        for k in range(n):
            for delta in tie_at.get(k, ()):
                t = int(logical[order[ipiv[k] + delta]])
                assert t > k
                add_r.append(t)
                add_c.append(k)
                add_v.append(1.0 if rng.random() < 0.5 else -1.0)
            p = ipiv[k]
            order[k], order[p] = order[p], order[k]
        key = np.asarray(add_r) * n + np.asarray(add_c)
        drop = np.isin(Lr * n + Lc, key)
        Lr = np.concatenate([Lr[~drop], add_r])
        Lc = np.concatenate([Lc[~drop], add_c])
        Lv = np.concatenate([Lv[~drop], add_v])
    on = d != 0
    Ur = np.concatenate([np.nonzero(on)[0], Ur])
    Uc = np.concatenate([np.nonzero(on)[0], Uc])
    Uv = np.concatenate([d[on], Uv])
    return Case(n, ipiv, Lr.astype(np.int64), Lc.astype(np.int64), Lv, Ur.astype(np.int64), Uc.astype(np.int64), Uv,
                zero_pivots)


def wilkinson(n):
    """The classic: 1 on the diagonal, -1 below it, 1 in the last column.  Every step ties (|L| = 1 below the diagonal)
    and none exchanges; U = I except its last column, 2^k.  Exact up to n = 128 (2^127)."""
    assert 1 <= n <= 128
    Lr, Lc = np.tril_indices(n, -1)
    Ur = np.concatenate([np.arange(n - 1), np.arange(n)])
    Uc = np.concatenate([np.arange(n - 1), np.full(n, n - 1)])
    Uv = np.concatenate([np.ones(n - 1), 2.0 ** np.arange(n)])
    case = Case(n, np.arange(n), Lr, Lc, -np.ones(len(Lr)), Ur, Uc, Uv)
    case.M = np.eye(n) - np.tril(np.ones((n, n)), -1)
    case.M[:, -1] = 1.0
    return case


def banded_wilkinson(n, band):
    """L = I - (the first `band` subdiagonals), U = I + ones in the last column: every step ties |L| = 1 across the
    whole band and none exchanges; the last column of M is small integers, so it is exact at any n."""
    j = np.arange(n)
    Lr = np.concatenate([j[s:] for s in range(1, band + 1)])
    Lc = np.concatenate([j[:n - s] for s in range(1, band + 1)])
    Ur = np.concatenate([j, j[:-1]])
    Uc = np.concatenate([j, np.full(n - 1, n - 1)])
    return Case(n, np.arange(n), Lr, Lc, -np.ones(len(Lr)), Ur, Uc, np.ones(len(Ur)))


def exact_inverse(n, seed, per=4, swap_prob=0.75, dense=True, first_swap=False):
    """M = Q (I + N1) D (I + N2) with N1 strictly lower, N2 strictly upper, N1^2 = N2^2 = 0 term by term (each maps rows
    of one parity from columns of the other), D a power-of-two diagonal.  Returns (case, M^-1):
    M^-1 = (I - N2) D^-1 (I - N1) Q^T exactly, dense float64 or (with dense=False) as (rows, cols, values)."""
    rng = np.random.default_rng(seed)
    base = generic(n, seed, per=per, swap_prob=swap_prob, first_swap=first_swap)
    # rows of one parity from columns of the other: N1's columns and N2's rows share a parity (the trailing updates
    # L21 U12 have product terms), N2's columns share the last column's (U keeps its last column)
    q = (n - 1) % 2
    lk = (base.Lr % 2 == q) & (base.Lc % 2 != q)
    off = base.Ur != base.Uc
    uk = ~off | ((base.Ur % 2 != q) & (base.Uc % 2 == q))
    # D in 1/4 .. 4 so that D^-1 and the products stay short
    d = np.ldexp(np.where(rng.random(n) < 0.5, -1.0, 1.0), rng.integers(-2, 3, n))
    Ur, Uc, Uv = base.Ur[uk], base.Uc[uk], base.Uv[uk].copy()
    on = Ur == Uc
    Uv[on] = d[Ur[on]]
    Uv[~on] = Uv[~on] * d[Ur[~on]]                       # U = D (I + N2): row k of N2 scaled by D[k]
    case = Case(n, base.ipiv, base.Lr[lk], base.Lc[lk], base.Lv[lk], Ur, Uc, Uv)
    # (I - N2) . D^-1 (I - N1), then Q^T as a column permutation
    i = np.arange(n)
    off = ~on
    yr, yc, yv = (np.concatenate([i, case.Lr]), np.concatenate([i, case.Lc]),
                  np.concatenate([1.0 / d, -case.Lv / d[case.Lr]]))
    ar, ac, av = (np.concatenate([i, Ur[off]]), np.concatenate([i, Uc[off]]),
                  np.concatenate([np.ones(n), -Uv[off] / d[Ur[off]]]))
    zr, zc, zv = _spmm(n, ar, ac, av, yr, yc, yv)
    coords = (zr, case.perm[zc], zv)
    if not dense:
        return case, coords
    inv = np.zeros((n, n))
    inv[coords[0], coords[1]] = coords[2]
    return case, inv


def trailing_coverage(case, nb=64, tile=128):
    """How the blocked factorization's rank-nb updates reach the trailing matrix, rows taken in their physical order at
    each panel (the exchanges move them; columns never move).  Returns (the panels with a trailing block, those whose
    U12 has an entry in the trailing block's last column tile, the fraction of the tile x tile blocks of the matrix
    below and right of the first tile that some panel's L21 U12 reaches with a nonzero product term)."""
    n = case.n
    nbk = (n + tile - 1) // tile
    hit = np.zeros((nbk, nbk), bool)
    order = np.arange(n, dtype=np.int64)              # position -> row of M
    where = np.arange(n, dtype=np.int64)              # row of M -> position
    lo = np.argsort(case.Lc, kind="stable")
    lr, lc = case.Lr[lo], case.Lc[lo]
    uo = np.argsort(case.Ur, kind="stable")
    ur, uc = case.Ur[uo], case.Uc[uo]
    panels = reach_last = 0
    for k0 in range(0, n, nb):
        k1 = min(n, k0 + nb)
        for k in range(k0, k1):
            p = int(case.ipiv[k])
            if p != k:
                a, b = order[k], order[p]
                order[k], order[p] = b, a
                where[b], where[a] = k, p
        if k1 >= n:
            break
        panels += 1
        ls, le_ = np.searchsorted(lc, [k0, k1])
        us, ue = np.searchsorted(ur, [k0, k1])
        rows, rcol = lr[ls:le_], lc[ls:le_]
        sel = rows >= k1
        rows, rcol = where[case.perm[rows[sel]]], rcol[sel]
        cols, crow = uc[us:ue], ur[us:ue]
        sel = cols >= k1
        cols, crow = cols[sel], crow[sel]
        last = k1 + tile * ((n - k1 - 1) // tile)
        reach_last += bool((cols >= last).any())
        R = np.zeros((k1 - k0, nbk), np.float32)
        R[rcol - k0, rows // tile] = 1.0
        Cm = np.zeros((k1 - k0, nbk), np.float32)
        Cm[crow - k0, cols // tile] = 1.0
        hit |= (R.T @ Cm) > 0
    frac = float(hit[1:, 1:].mean()) if nbk > 1 else 1.0
    return panels, reach_last, frac


# the large cases of tests/test_gpu_linalg_exact.py, pinned on the CPU by tests/test_linalg_reference_cpu.py
LARGE_GETRF = [8193, 16384, 16385, 32769, 46341]
LARGE_ND = [16384, 16385]
LARGE_SOLVE = 46341


def large_case(n, seed, parity=None):
    """generic() as the large tests use it: 8 partners per column of L and row of U, and a first step that exchanges
    rows (perm_kernel's global branch would otherwise drop a no-op)."""
    return generic(n, seed=seed, per=8, parity=parity, first_swap=True)


def large_getrf_case(n):
    return large_case(n, n)


def large_nd_case(n):
    return large_case(n, n + 1, parity=n % 2)


def large_solve_case():
    return large_case(LARGE_SOLVE, 5)


def large_inverse_case(n):
    """(case, coordinates of M^-1) of the exact-inverse family for the large inv tests"""
    return exact_inverse(n, n + 2, per=16, dense=False, first_swap=True)
