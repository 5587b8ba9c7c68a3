"""The structural constructors on device handles (spl_matrix_kronecker, _assemble_blocks, _take_diag_dev, _diag_dev):
what they answer before the device is touched.  Argument checks come first, so these hold with or without a GPU."""
import ctypes as C

import numpy as np

SYMBOLS = ("spl_matrix_kronecker", "spl_matrix_assemble_blocks", "spl_matrix_take_diag_dev", "spl_matrix_diag_dev")


def _not_a_handle():
    """memory that is readable where a handle's magic would be, and is none"""
    return C.create_string_buffer(256)


def test_the_four_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes, name
    for name in ("kronecker", "assemble", "hcat", "vcat", "from_blocks", "from_blocks_diag", "block_diag",
                 "take_diag_dev", "take_diag", "diag_dev", "ident"):
        assert callable(getattr(pkg.DeviceMatrix, name)), name


def test_null_and_foreign_operands_are_invalid_handles(pkg):
    F = pkg._ffi
    L = F.lib()
    junk = _not_a_handle()
    for a, b in ((None, None), (junk, None), (None, junk), (junk, junk)):
        h = C.c_void_p(0x1234)  # must not be read, and is not written: the operands are refused first
        assert L.spl_matrix_kronecker(a, b, C.byref(h)) == F.SPL_ERROR_invalid_handle
    out = (C.c_double * 4)()
    assert L.spl_matrix_take_diag_dev(None, out, None) == F.SPL_ERROR_invalid_handle
    assert L.spl_matrix_take_diag_dev(junk, out, None) == F.SPL_ERROR_invalid_handle
    off = np.zeros(2, dtype=np.int64)
    for blocks in ((None, None), (C.addressof(junk), None), (C.addressof(junk), C.addressof(junk))):
        hs = (C.c_void_p * 2)(*blocks)
        h = C.c_void_p()
        st = L.spl_matrix_assemble_blocks(2, hs, F.p_i64(off), F.p_i64(off), 4, 4, C.byref(h))
        assert st == F.SPL_ERROR_invalid_handle and not h.value


def test_diag_dev_checks_its_arguments_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    h = C.c_void_p(0x1234)
    assert L.spl_matrix_diag_dev(-1, None, 1, C.byref(h)) == F.SPL_ERROR_n_nonpositive
    assert not h.value  # the output is cleared even when the call is refused
    for width in (0, 3, -1):
        h = C.c_void_p(0x1234)
        assert L.spl_matrix_diag_dev(5, None, width, C.byref(h)) == F.SPL_ERROR_argument_missing
        assert not h.value
    assert L.spl_matrix_diag_dev(5, None, 1, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_diag_dev(-1, None, 7, None) == F.SPL_ERROR_argument_missing  # no output: nothing else is looked at


def test_assemble_blocks_without_blocks_checks_shape_and_output(pkg):
    F = pkg._ffi
    L = F.lib()
    h = C.c_void_p()
    assert L.spl_matrix_assemble_blocks(-1, None, None, None, 3, 3, C.byref(h)) == F.SPL_ERROR_n_nonpositive
    assert L.spl_matrix_assemble_blocks(0, None, None, None, 3, 3, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_assemble_blocks(0, None, None, None, -3, 3, C.byref(h)) == F.SPL_ERROR_n_nonpositive
    assert not h.value


def test_a_well_formed_diag_dev_needs_a_device(pkg):
    F = pkg._ffi
    L = F.lib()
    h = C.c_void_p(0x1234)
    st = L.spl_matrix_diag_dev(5, None, 1, C.byref(h))
    if F.device_count() < 1:
        assert st == F.SPL_ERROR_device and not h.value
        h = C.c_void_p(0x1234)
        assert L.spl_matrix_assemble_blocks(0, None, None, None, 3, 3, C.byref(h)) == F.SPL_ERROR_device and not h.value
    else:
        assert st == F.SPL_OK and h.value
        L.spl_matrix_free(C.byref(h))
        assert not h.value
