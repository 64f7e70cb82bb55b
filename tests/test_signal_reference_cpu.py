"""CPU-tier checks of what the 2-D correlation tests compare with (tests/signal_family.py): ref2d equals scipy.signal for
every mode, boundary and function — windows larger than the image, even extents, 1 x N and N x 1, 'valid' with the operands
swapped; the separable closed form equals ref2d; np_correlate2d_shape (no device needed) reports ref2d's shapes and refuses
what it must."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import signal_family as F

PAIRS = [((5, 7), (3, 3)), ((4, 4), (2, 2)), ((3, 3), (7, 9)), ((1, 9), (1, 4)), ((9, 1), (4, 1)), ((6, 5), (4, 2)), ((2, 3), (5, 8)),
         ((3, 9), (3, 2)), ((2, 2), (11, 13)), ((4, 4), (4, 4)), ((1, 1), (1, 1)), ((7, 6), (1, 1)), ((3, 9), (5, 2))]
COMBOS = list(itertools.product(F.MODES, F.BOUNDARIES, (0, 1)))


def test_ref2d_is_scipy_for_all_18_combinations():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    checked = raised = 0
    for (sa, sb), (mode, boundary, flip) in itertools.product(PAIRS, COMBOS):
        a, b = F.exact(rng, sa, sb)
        fill = float(rng.integers(-8, 9)) if boundary == "fill" else 0.0
        call = signal.convolve2d if flip else signal.correlate2d
        try:
            want = call(a, b, mode, boundary, fill)
        except ValueError as e:
            assert "For 'valid' mode, one must be at least as large as the other in every dimension" in str(e)   # (the reference says "one input")
            with pytest.raises(ValueError):
                F.ref2d(a, b, mode, boundary, fill, flip)
            raised += 1
            continue
        got = F.ref2d(a, b, mode, boundary, fill, flip)
        assert got.shape == want.shape == F.out_shape(sa, sb, mode), (sa, sb, mode)
        assert np.array_equal(got, want), (sa, sb, mode, boundary, flip)
        checked += 1
    assert checked >= 200 and raised >= 6
    # 'valid' swapped: a convolution is symmetric in its operands, a correlation comes out reversed
    a, b = F.exact(rng, (2, 3), (6, 8))
    assert np.array_equal(F.ref2d(a, b, "valid", flip=1), F.ref2d(b, a, "valid", flip=1))
    assert np.array_equal(F.ref2d(a, b, "valid", flip=0), signal.correlate2d(a, b, "valid"))
    # fp32 SciPy on the exact family is its own fp64 result: the family is exact in any order
    a, b = F.exact(rng, (60, 50), (31, 29))
    assert np.array_equal(signal.correlate2d(a, b, "same", "symm").astype(np.float64), F.ref2d(a, b, "same", "symm"))


def test_the_separable_closed_form_is_ref2d():
    rng = np.random.default_rng(1)
    for mode, boundary, flip in COMBOS:
        for sb in ((3, 3), (4, 7), (9, 12)):
            if boundary == "fill" and mode != "valid":
                continue
            a, u, v = F.separable(rng, 9, 12)
            b = rng.integers(-4, 5, size=sb).astype(np.float32)
            assert np.array_equal(a, u[:, None] + v[None, :])
            want = F.ref2d(a, b, mode, boundary, 0.0, flip)
            got = F.separable_expected(u, v, b, mode, boundary, flip)
            assert got.dtype == np.float32 and np.array_equal(got, want), (mode, boundary, flip, sb)


def test_gamma_is_the_inner_product_bound():
    assert F.gamma(9) == 10 * 2.0 ** -24 / (1 - 10 * 2.0 ** -24)
    assert F.gamma(255 * 255) < 4e-3


def test_shape_entry_point_needs_no_device_and_matches_ref2d():
    from numpower_amd import _lib
    lib = _lib.load()
    lib.np_last_error.restype = C.c_char_p
    oh, ow = C.c_size_t(), C.c_size_t()
    for (sa, sb), mode in itertools.product(PAIRS + [((16384, 16384), (255, 255)), ((3, 1000), (1000, 3))], F.MODES):
        rc = lib.np_correlate2d_shape(sa[0], sa[1], sb[0], sb[1], F.MODE_FLAG[mode], C.byref(oh), C.byref(ow))
        try:
            want = F.out_shape(sa, sb, mode)
        except ValueError as e:
            assert rc == -1 and lib.np_last_error().decode() == str(e)
            continue
        assert rc == _lib.NP_OK and (oh.value, ow.value) == want, (sa, sb, mode)
    big = 2 ** 31 - 1
    assert lib.np_correlate2d_shape(big, 1, 1, 1, 1, C.byref(oh), C.byref(ow)) == _lib.NP_OK and oh.value == big
    for args in ((big + 1, 1, 1, 1, 1), (1, 1, 1, big + 1, 1), (big, 1, 2, 1, 2), (1, big - 1, 1, 3, 2),      # beyond int shapes
                 (0, 4, 2, 2, 1), (4, 4, 2, 0, 2), (4, 4, 2, 2, 3), (4, 4, 2, 2, -1), (4, 1, 2, 2, 0)):
        assert lib.np_correlate2d_shape(*args, C.byref(oh), C.byref(ow)) == -1, args
        assert lib.np_last_error()
    assert lib.np_correlate2d_shape(4, 4, 2, 2, 1, None, C.byref(ow)) == -1 and lib.np_correlate2d_shape(4, 4, 2, 2, 1, C.byref(oh), None) == -1
