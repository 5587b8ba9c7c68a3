"""Windows and selections of device handles (spl_matrix_submatrix, spl_matrix_select): what they answer before the
device is touched.  Argument checks come first, so these hold with or without a GPU; the checks that need a real
handle (negative arguments, the two guards, row blocks, index arrays) are in tests/test_gpu_submatrix.py."""
import ctypes as C

SYMBOLS = ("spl_matrix_submatrix", "spl_matrix_select")


def _not_a_handle():
    """memory that is readable where a handle's magic would be, and is none"""
    return C.create_string_buffer(256)


def test_the_two_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(L.spl_matrix_submatrix.argtypes) == 6 and len(L.spl_matrix_select.argtypes) == 8


def test_the_python_surface_exists(pkg):
    for name in ("submatrix", "select", "__getitem__"):
        assert callable(getattr(pkg.DeviceMatrix, name)), name
    assert callable(pkg.subMatrix) and callable(pkg.sparse.subMatrix)
    doc = pkg.subMatrix.__doc__
    # the three defects of Sparse.hs:704-729 are named, and what is computed instead
    assert "704-729" in doc and "U.slice" in doc and "not shifted" in doc and "computePtrs" in doc
    assert "documented operation" in doc


def test_null_and_foreign_operands_are_invalid_handles(pkg):
    F = pkg._ffi
    L = F.lib()
    for operand in (None, _not_a_handle()):
        h = C.c_void_p(0x1234)  # must not be read, and is not written: the operand is refused first
        assert L.spl_matrix_submatrix(operand, 0, 0, 1, 1, C.byref(h)) == F.SPL_ERROR_invalid_handle
        assert h.value == 0x1234
        bad = C.c_int64(-7)
        assert L.spl_matrix_select(operand, 1, None, 1, None, 4, C.byref(h), C.byref(bad)) == F.SPL_ERROR_invalid_handle
        assert h.value == 0x1234 and bad.value == -7
        # nothing else is looked at before the handle: not the output, not the counts, not the width
        assert L.spl_matrix_submatrix(operand, -1, -1, -1, -1, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_matrix_select(operand, -1, None, -1, None, 3, None, None) == F.SPL_ERROR_invalid_handle


def test_a_missing_output_is_an_argument_missing(pkg):
    """HC == NULL comes second.  A handle's magic is its first four bytes ("SPLM" as a little-endian word), so a buffer
    that starts with them passes the first check and nothing behind them is read before the second"""
    F = pkg._ffi
    L = F.lib()
    fake = C.create_string_buffer(b"MLPS" + bytes(508))
    assert L.spl_matrix_submatrix(fake, 0, 0, 1, 1, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_submatrix(fake, -1, -1, -1, -1, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_select(fake, 1, None, 1, None, 4, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_select(fake, -1, None, -1, None, 3, None, None) == F.SPL_ERROR_argument_missing


def test_getitem_refuses_what_is_neither_a_window_nor_a_selection(pkg):
    """the dispatch of DeviceMatrix[...] is decided on the key alone: no handle is touched for a refused key"""
    import pytest
    H = pkg.DeviceMatrix(None)
    for key in ((slice(None, None, 2), slice(None)), (slice(None), slice(0, 4, 3)), 3, (1, 2), (slice(None),),
                (slice(0, 2), [0, 1]), ([0, 1], slice(0, 2)), ([True, False], [0]), ([[0, 1]], [0]), ([0.5], [0])):
        with pytest.raises(TypeError):
            H[key]
