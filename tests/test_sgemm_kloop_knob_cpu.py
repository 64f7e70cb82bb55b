"""The K-loop knob of the 256 x 128 LDS-DMA kernels (include/np_hip_debug.h) is host state: the three codes are accepted, the rest of
the reserved range is refused, and the launch counter answers without a device."""
import ctypes as C


def test_kloop_knob_codes_and_counter():
    from numpower_amd import _lib
    lib = _lib.load()
    lib.np_last_error.restype = C.c_char_p
    try:
        for code in (-31, -32, -33):
            assert lib.np_sgemm_set_variant(code) == 0, code
        for code in (-34, -39):
            assert lib.np_sgemm_set_variant(code) != 0 and b"not assigned" in lib.np_last_error()
    finally:
        assert lib.np_sgemm_set_variant(-33) == 0
    out = (C.c_ulonglong * 2)(7, 7)
    assert lib.np_sgemm_debug_kloop_stats(out) == 0 and list(out) == [0, 0]   # nothing was launched in this process
    assert lib.np_sgemm_debug_kloop_stats(None) != 0
    assert lib.np_sgemm_debug_ld(0, 4, 4, None, 4, None, 4, None, 4) != 0
