"""The exact reduction family (tests/reduce_family.py) on the CPU: its expectations equal the oracle's sequential loops bit for
bit, equal fp32 accumulation in several different orders (so any correct device order returns them too), follow the
reference's NaN rule for min / max, and it refuses parameters that leave the exact range.  Also: the probes the device tests
assert their paths with are declared, exported and prototyped."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import reduce_family as rf

ROOT = Path(__file__).resolve().parent.parent

SHAPES = [((1,), None), ((9,), None), ((4097,), None), ((100003,), None), ((7, 4097), 1), ((4001, 3), 0), ((3, 1001, 5), 1),
          ((300, 260), 0), ((257, 33), 1), ((2, 40000, 3), 1)]


def _same(got, want):
    return rf.mismatches(got, want).size == 0


def _orders(v, op):
    """fp32 accumulation of the (outer, n, inner) view along n in four orders: forward, reversed, pairwise (numpy's own), and
    a seeded permutation folded in two interleaved halves."""
    f = {"sum": np.add, "prod": np.multiply}[op]
    one = np.float32(0 if op == "sum" else 1)

    def seq(a):
        acc = np.full((a.shape[0], a.shape[2]), one, np.float32)
        for i in range(a.shape[1]):
            acc = f(acc, a[:, i, :], dtype=np.float32)
        return acc
    perm = np.random.default_rng(5).permutation(v.shape[1])
    p = v[:, perm, :]
    return [seq(v), seq(v[:, ::-1, :]), f.reduce(v, axis=1, dtype=np.float32), f(seq(p[:, 0::2, :]), seq(p[:, 1::2, :]), dtype=np.float32)]


@pytest.mark.parametrize("shape,axis", SHAPES)
def test_family_equals_oracle_and_every_order(shape, axis, oracle):
    n = int(np.prod(shape)) if axis is None else shape[axis]
    arrays = {"sum": rf.ints(shape, 11, 4, axis), "prod": rf.prods(shape, axis, 12)}
    arrays["mean"] = arrays["sum"]
    for op, x in arrays.items():
        want = rf.expected(x, axis, op)
        got = oracle.reduce_all(op, x) if axis is None else oracle.reduce_axis(op, x, axis)
        assert _same(got, want), (op, shape, axis)
        if op != "mean" and n <= 5000:
            for k, r in enumerate(_orders(rf._slices(x, axis), op)):
                assert _same(r.reshape(want.shape), want), (op, shape, axis, "order %d" % k)
    # a changed element always shows: drop one, double one
    x = arrays["sum"].copy()
    total = rf.expected(x, None, "sum")
    x.reshape(-1)[x.size // 2] *= 2
    assert rf.expected(x, None, "sum") != total
    x = arrays["prod"].copy()
    want = rf.expected(x, axis, "prod")
    x.reshape(-1)[x.size // 3] = 1.0          # "dropped"
    with pytest.raises(ValueError):
        rf.expected(x, axis, "prod")          # (+1 is not in the family: nothing can hide behind it)
    x.reshape(-1)[x.size // 3] = 2.0 if arrays["prod"].reshape(-1)[x.size // 3] != 2.0 else -1.0
    assert rf.mismatches(rf.expected(x, axis, "prod"), want).size >= 1


@pytest.mark.parametrize("n", [2 ** 20, 4200003])
def test_flat_bounds_of_the_issue_hold(n, oracle):
    """amp = 4 up to 2^20 along an axis and amp = 3 for 4 200 003 flat elements stay inside 2^24; the oracle's left-to-right
    fp32 loop and numpy's pairwise one return the int64 sum."""
    x = rf.ints((n,), 3, 4 if n == 2 ** 20 else 3)
    want = rf.expected(x, None, "sum")
    assert int(want) == int(x.astype(np.int64).sum())
    assert _same(oracle.reduce_all("sum", x), want) and _same(np.add.reduce(x, dtype=np.float32), want)
    assert _same(np.add.reduce(x[::-1], dtype=np.float32), want)
    assert _same(oracle.reduce_all("mean", x), rf.expected(x, None, "mean"))


@pytest.mark.parametrize("shape,axis", SHAPES)
def test_extremes_and_specials_follow_the_reference_loop(shape, axis, oracle):
    n = int(np.prod(shape)) if axis is None else shape[axis]
    pos = rf.positions(n)
    assert pos[0] == 0 and pos[-1] == n - 1 and all(0 <= p < n for p in pos)
    seen_hi, seen_lo = set(), set()
    bg = None
    for rnd in range(min(rf.extreme_rounds(shape, axis, pos), 40)):
        x, bg = rf.extremes(shape, axis, pos, 21, rnd, bg)
        v = rf._slices(x, axis)
        assert ((v == 2.0).sum(axis=1) == 1).all() and ((v == -2.0).sum(axis=1) == (1 if n > 1 else 0)).all()
        seen_hi.update(np.argmax(v, axis=1).reshape(-1).tolist())
        seen_lo.update(np.argmin(v, axis=1).reshape(-1).tolist())
        assert (rf.expected(x, axis, "max") == 2.0).all() and (rf.expected(x, axis, "min") == (-2.0 if n > 1 else 2.0)).all()
        if axis is None:
            assert _same(oracle.reduce_all("max", x), rf.expected(x, None, "max"))
            assert _same(oracle.reduce_all("min", x), rf.expected(x, None, "min"))
    if rf.extreme_rounds(shape, axis, pos) <= 40:
        assert seen_hi == set(pos) and (n == 1 or len(seen_lo) >= len(pos) - 1)
    base = rf.ints(shape, 31, 3, axis)
    seen = set()
    for rnd in range(8):
        x, kinds = rf.specials(base, axis, pos, 0, rnd)
        seen.update(np.unique(kinds).tolist())
        v = rf._slices(x, axis)
        first_nan = np.isnan(v[:, 0, :]).reshape(kinds.shape)
        any_nan = np.isnan(v).any(axis=1).reshape(kinds.shape)
        for op in ("min", "max"):
            want = rf.expected(x, axis, op)
            assert _same(want, rf.minmax_loop(x, axis, op)) and _same(want, rf._minmax_closed(x, axis, op))
            assert (np.isnan(want) == first_nan).all()          # NaN exactly where position 0 is one
            if axis is None:
                assert _same(oracle.reduce_all(op, x), want), (op, shape, int(kinds))
        for op in ("sum", "mean"):
            want = rf.expected(x, axis, op)
            both = ((v == np.inf).any(axis=1) & (v == -np.inf).any(axis=1)).reshape(kinds.shape)
            assert (np.isnan(want) == (any_nan | both)).all()
            assert (want[kinds == rf.FINITE] == rf.expected(base, axis, op)[kinds == rf.FINITE]).all()   # neighbours untouched
            got = oracle.reduce_all(op, x) if axis is None else oracle.reduce_axis(op, x, axis)
            assert _same(got, want), (op, shape, axis)
        xp, _ = rf.specials(rf.prods(shape, axis, 32), axis, pos, 0, rnd)
        got = oracle.reduce_all("prod", xp) if axis is None else oracle.reduce_axis("prod", xp, axis)
        assert _same(got, rf.expected(xp, axis, "prod")), ("prod", shape, axis)
    assert seen >= (set(rf.SPECIAL_KINDS) if n > 1 else {rf.NAN_FIRST, rf.INF_ALONE})


def test_nan_rule_in_words(oracle):
    """Position 0 decides: NaN there is the result, NaN anywhere else is ignored, all-NaN gives NaN."""
    nan = np.float32(np.nan)
    for op, pick in (("max", 3.0), ("min", -5.0)):
        assert np.isnan(rf.expected(np.array([nan, 1, 3, -5], np.float32), None, op))
        assert rf.expected(np.array([1, nan, 3, -5, nan], np.float32), None, op) == pick
        assert np.isnan(rf.expected(np.array([nan, nan, nan], np.float32), None, op))
        assert np.isnan(oracle.reduce_all(op, np.array([nan, 1, 3, -5], np.float32)))
        assert oracle.reduce_all(op, np.array([1, nan, 3, -5, nan], np.float32)) == pick
    x = rf.zero_extremes((6, 50), 1, 4)
    assert (rf.expected(x, 1, "min") == 0.0).all() and (rf.expected(-x, 1, "max") == 0.0).all()
    assert {0, 0x80000000} == set(rf.bits(rf.expected(x, 1, "min")).tolist())     # "the first one": both signs occur
    assert rf.mismatches(np.zeros(6, np.float32), rf.expected(x, 1, "min")).size > 0
    assert rf.mismatches(np.zeros(6, np.float32), rf.expected(x, 1, "min"), np.ones(6, bool)).size == 0


def test_family_refuses_what_is_not_exact():
    with pytest.raises(ValueError):
        rf.ints((2 ** 23,), 1, 4)                     # could reach 2^25
    with pytest.raises(ValueError):
        rf.ints((3, 2 ** 23), 1, 4, axis=1)
    rf.ints((2 ** 23, 2), 1, 4, axis=1)               # the same elements in short slices are fine
    with pytest.raises(ValueError):
        rf.ints((4,), 1, 0)
    with pytest.raises(ValueError):
        rf.expected(np.array([1.5, 2.0], np.float32), None, "sum")
    with pytest.raises(ValueError):
        rf.expected(np.full(2 ** 23, 2, np.float32), None, "mean")
    with pytest.raises(ValueError):
        rf.expected(np.array([3.0, -1.0], np.float32), None, "prod")
    with pytest.raises(ValueError):
        rf.expected(np.full(61, 2.0, np.float32), None, "prod")
    with pytest.raises(ValueError):
        rf.extremes((5,), None, [5], 1)
    with pytest.raises(ValueError):
        rf.expected(np.ones(3, np.float32), None, "median")
    k = rf.prods((64, 500), 1, 9)
    assert len({tuple(r) for r in np.stack([(k == 2).sum(1), (k == 0.5).sum(1)], 1).tolist()}) > 32   # neighbouring slices differ


def test_reduce_probes_are_declared_exported_and_prototyped():
    from numpower_amd import _lib
    header = (ROOT / "include" / "np_hip_debug.h").read_text()
    lib = _lib.load()
    for name in ("np_debug_reduce_last_path", "np_debug_chain_reduce_last_path"):
        assert "int %s(unsigned *host_mask);" % name in header
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert "int np_debug_cus(int *host_cus);" in header and hasattr(lib, "np_debug_cus") and "np_debug_cus" in _lib.PROTOTYPES
    for prefix, count in (("NP_REDUCE_PATH_", 15), ("NP_CHAIN_PATH_", 9)):
        values = [int(v, 16) for v in re.findall(r"#define %s\w+ (0x[0-9a-f]+)u" % prefix, header)]
        assert len(values) == count and len(set(values)) == count and all(v & (v - 1) == 0 for v in values)   # one bit each
    assert "np_debug_reduce_last_path" not in (ROOT / "include" / "np_hip.h").read_text()
