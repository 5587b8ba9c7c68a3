"""The entry-wise layer on device handles (spl_matrix_map, _scale_rows_cols, _filter, _band, _reduce_dev, _norm): what
the calls answer before the device is touched.  Argument checks come first, so these hold with or without a GPU; what
needs a real handle (imaginary scalars on real handles, row blocks, NULL outputs of non-empty axes, the vectors' dtypes)
is in tests/test_gpu_entrywise.py."""
import ctypes as C

SYMBOLS = {"spl_matrix_map": 4, "spl_matrix_scale_rows_cols": 4, "spl_matrix_filter": 4, "spl_matrix_band": 4,
           "spl_matrix_reduce_dev": 5, "spl_matrix_norm": 3}
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _not_a_handle():
    """memory that is readable where a handle's magic would be, and is none"""
    return C.create_string_buffer(256)


def _magic_only():
    """A handle's magic is its first four bytes ("SPLM" as a little-endian word): a buffer that starts with them passes
    the first check.  Everything behind them is zero: a real 0 x 0 matrix on device 0 to whoever reads on"""
    return C.create_string_buffer(b"MLPS" + bytes(508))


def test_the_six_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes and len(fn.argtypes) == nargs, name
    F = pkg._ffi
    assert (F.SPL_MAP_negate, F.SPL_MAP_abs, F.SPL_MAP_signum, F.SPL_MAP_conj, F.SPL_MAP_real, F.SPL_MAP_imag,
            F.SPL_MAP_scale) == tuple(range(7))
    assert (F.SPL_KEEP_nonzero, F.SPL_KEEP_abs_above, F.SPL_REDUCE_abs_sum, F.SPL_REDUCE_abs_max) == (0, 1, 0, 1)
    assert (F.SPL_NORM_one, F.SPL_NORM_inf, F.SPL_NORM_fro, F.SPL_NORM_max) == (0, 1, 2, 3)


def test_the_header_names_the_same_codes(pkg):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sparse_linear_hip.h")).read()
    codes = dict(re.findall(r"^#define (SPL_(?:MAP|KEEP|REDUCE|NORM)_\w+) (\d+)$", text, re.M))
    assert len(codes) == 15
    for name, value in codes.items():
        assert getattr(pkg._ffi, name) == int(value), name


def test_the_python_surface_exists(pkg):
    D = pkg.DeviceMatrix
    for name in ("map", "negate", "abs", "signum", "conj", "real", "imag", "scale", "__neg__", "__abs__",
                 "scale_rows_cols", "drop_zeros", "drop_small", "band", "tril", "triu", "abs_sums", "abs_max", "norm"):
        assert callable(getattr(D, name)), name
    assert sorted(D.MAP_OPS) == ["abs", "conj", "imag", "negate", "real", "scale", "signum"]
    # the host Matrix keeps its numpy forms
    assert callable(pkg.sparse.cmap) and callable(pkg.sparse.scale) and callable(pkg.Matrix.signum)


def test_refused_names_touch_no_handle(pkg):
    """the Python forms decide on their own arguments before the handle is looked at"""
    import pytest
    H = pkg.DeviceMatrix(None)
    with pytest.raises(ValueError):
        H.map("sqrt")
    with pytest.raises(ValueError):
        H.map("scale")
    with pytest.raises(ValueError):
        H.norm(2)
    with pytest.raises(ValueError):
        H.abs_sums(2)


def _calls(L, operand, h, r):
    """every call once on `operand` with legal codes; h: void** or None, r: double* or None"""
    s = (C.c_double * 2)(2.0, 0.0)
    return [L.spl_matrix_map(operand, 0, None, h), L.spl_matrix_map(operand, 6, s, h),
            L.spl_matrix_scale_rows_cols(operand, None, None, h),
            L.spl_matrix_filter(operand, 0, None, h), L.spl_matrix_filter(operand, 1, (C.c_double * 1)(0.5), h),
            L.spl_matrix_band(operand, -1, 1, h), L.spl_matrix_band(operand, I64_MIN, I64_MAX, h),
            L.spl_matrix_norm(operand, 2, r)]


def test_null_and_foreign_operands_are_invalid_handles(pkg):
    F = pkg._ffi
    L = F.lib()
    for operand in (None, _not_a_handle()):
        h = C.c_void_p(0x1234)  # must not be read, and is not written: the operand is refused first
        r = C.c_double(-7.5)
        assert set(_calls(L, operand, C.byref(h), C.byref(r))) == {F.SPL_ERROR_invalid_handle}
        assert h.value == 0x1234 and r.value == -7.5
        for what, axis in ((0, 0), (1, 1), (9, 9)):
            assert L.spl_matrix_reduce_dev(operand, what, axis, None, None) == F.SPL_ERROR_invalid_handle
        # nothing else is looked at before the handle: not the outputs, not the codes, not the tolerance
        assert set(_calls(L, operand, None, None)) == {F.SPL_ERROR_invalid_handle}
        assert L.spl_matrix_map(operand, 99, None, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_matrix_filter(operand, 99, (C.c_double * 1)(-1.0), None) == F.SPL_ERROR_invalid_handle
        assert L.spl_matrix_norm(operand, 99, None) == F.SPL_ERROR_invalid_handle


def test_a_missing_output_is_an_argument_missing(pkg):
    """HC == NULL (result == NULL for the norm) comes second, before the codes"""
    F = pkg._ffi
    L = F.lib()
    fake = _magic_only()
    assert set(_calls(L, fake, None, None)) == {F.SPL_ERROR_argument_missing}
    assert L.spl_matrix_map(fake, 99, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_filter(fake, 99, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_norm(fake, 99, None) == F.SPL_ERROR_argument_missing


def test_unknown_codes_are_argument_missing(pkg):
    F = pkg._ffi
    L = F.lib()
    fake = _magic_only()
    s = (C.c_double * 2)(2.0, 0.0)
    for code in (-1, 7, 99):
        h = C.c_void_p(0x1234)
        assert L.spl_matrix_map(fake, code, s, C.byref(h)) == F.SPL_ERROR_argument_missing
        assert not h.value  # *HC is cleared once the output is known to exist
    for code in (-1, 2, 99):
        h = C.c_void_p(0x1234)
        assert L.spl_matrix_filter(fake, code, (C.c_double * 1)(0.5), C.byref(h)) == F.SPL_ERROR_argument_missing
        assert not h.value
    out = (C.c_double * 4)()
    for what, axis in ((-1, 0), (2, 1), (0, -1), (1, 2), (0, 3), (99, 99)):
        assert L.spl_matrix_reduce_dev(fake, what, axis, out, None) == F.SPL_ERROR_argument_missing
    for code in (-1, 4, 99):
        r = C.c_double(-7.5)
        assert L.spl_matrix_norm(fake, code, C.byref(r)) == F.SPL_ERROR_argument_missing
        assert r.value == -7.5
    # scale without its scalar
    h = C.c_void_p(0x1234)
    assert L.spl_matrix_map(fake, F.SPL_MAP_scale, None, C.byref(h)) == F.SPL_ERROR_argument_missing
    # a vector off the 8-byte grid
    assert L.spl_matrix_scale_rows_cols(fake, C.c_void_p(0x1004), None, C.byref(h)) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_scale_rows_cols(fake, None, C.c_void_p(0x1004), C.byref(h)) == F.SPL_ERROR_argument_missing


def test_a_negative_or_nan_tolerance_is_argument_missing(pkg):
    F = pkg._ffi
    L = F.lib()
    fake = _magic_only()
    for tol in (-1.0, -5e-324, float("-inf"), float("nan")):
        h = C.c_void_p(0x1234)
        assert L.spl_matrix_filter(fake, F.SPL_KEEP_abs_above, (C.c_double * 1)(tol), C.byref(h)) == \
            F.SPL_ERROR_argument_missing
        assert not h.value
    h = C.c_void_p(0x1234)
    assert L.spl_matrix_filter(fake, F.SPL_KEEP_abs_above, None, C.byref(h)) == F.SPL_ERROR_argument_missing
