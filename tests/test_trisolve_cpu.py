"""Sparse triangular solves on device handles (spl_trisolve_analyze, _solve_dev, _solve, _info, _free): what the calls
answer before the device is touched.  Argument checks come first, so these hold with or without a GPU; what needs a real
handle and a real object is in tests/test_gpu_trisolve.py."""
import ctypes as C
import os
import re

import pytest

SYMBOLS = {"spl_trisolve_analyze": 4, "spl_trisolve_solve_dev": 8, "spl_trisolve_solve": 5, "spl_trisolve_info": 2}
CODES = {"SPL_TRI_lower": 0, "SPL_TRI_upper": 1, "SPL_DIAG_stored": 0, "SPL_DIAG_unit": 1, "SPL_OP_n": 0, "SPL_OP_t": 1,
         "SPL_OP_h": 2}


def _not_a_handle():
    """memory that is readable where a magic word would be, and holds none"""
    return C.create_string_buffer(256)


def _matrix_magic_only():
    """the first four bytes of a matrix handle ("SPLM" as a little-endian word), zeros behind them: a 0 x 0 matrix
    without row pointers to whoever reads on"""
    return C.create_string_buffer(b"MLPS" + bytes(508))


def test_the_five_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes and len(fn.argtypes) == nargs, name
    free = L.spl_trisolve_free
    assert free.restype is None and len(free.argtypes) == 1
    for name, value in CODES.items():
        assert getattr(pkg._ffi, name) == value, name


def test_the_header_names_the_same_codes(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sparse_linear_hip.h")).read()
    codes = dict(re.findall(r"^#define (SPL_(?:TRI|DIAG|OP)_\w+) (\d+)$", text, re.M))
    assert len(codes) == 7
    for name, value in codes.items():
        assert getattr(pkg._ffi, name) == int(value) == CODES[name], name


def test_the_python_surface_exists(pkg):
    assert callable(pkg.DeviceMatrix.triangular)
    T = pkg.sparse.TriangularSolver
    for name in ("solve", "solve_dev", "info", "free"):
        assert callable(getattr(T, name)), name
    assert sorted(T.UPLO) == ["lower", "upper"] and sorted(T.TRANS) == ["H", "N", "T"]
    assert callable(pkg.sparse.solveTriangular) and callable(pkg.solveTriangular)
    t = T(None)
    assert t.singular is False and T(None, 1).singular is True
    t.free()
    t.free()


def test_refused_names_touch_no_handle(pkg):
    """the Python forms decide on their own arguments before the handle is looked at"""
    H = pkg.DeviceMatrix(None)
    for uplo in ("L", "diagonal", 0, None):
        with pytest.raises(ValueError):
            H.triangular(uplo)
    T = pkg.sparse.TriangularSolver(None)
    for trans in ("n", "C", 0, None):
        with pytest.raises(ValueError):
            T.solve([1.0], trans)
        with pytest.raises(ValueError):
            T.solve_dev(0, 1, 0, 1, 1, trans)
        with pytest.raises(ValueError):
            pkg.solveTriangular(pkg.ident(2), [1.0, 1.0], trans=trans)
    # a good name on an object that holds nothing: the handle is looked at, and is none
    with pytest.raises(pkg.SparseLinearError):
        T.solve_dev(0, 1, 0, 1, 1, "N")
    with pytest.raises(pkg.SparseLinearError):
        H.triangular("upper")


def test_analyze_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    for operand in (None, _not_a_handle()):
        t = C.c_void_p(0x1234)  # not written: the operand is refused first
        assert L.spl_trisolve_analyze(operand, 0, 0, C.byref(t)) == F.SPL_ERROR_invalid_handle
        assert t.value == 0x1234
        assert L.spl_trisolve_analyze(operand, 9, 9, None) == F.SPL_ERROR_invalid_handle
    fake = _matrix_magic_only()
    assert L.spl_trisolve_analyze(fake, 0, 0, None) == F.SPL_ERROR_argument_missing
    for uplo, diag in ((-1, 0), (2, 0), (0, -1), (0, 2), (99, 99)):
        t = C.c_void_p(0x1234)
        assert L.spl_trisolve_analyze(fake, uplo, diag, C.byref(t)) == F.SPL_ERROR_argument_missing
        assert not t.value  # *T is cleared once the output is known to exist
    # a square "handle" without 32-bit row pointers
    t = C.c_void_p(0x1234)
    assert L.spl_trisolve_analyze(fake, 1, 1, C.byref(t)) == F.SPL_ERROR_invalid_matrix
    assert not t.value


def test_solve_info_and_free_refuse_what_is_no_object(pkg):
    F = pkg._ffi
    L = F.lib()
    buf = (C.c_double * 4)()
    info = (C.c_int64 * 8)(*([-7] * 8))
    # a matrix handle's magic is not this object's
    for operand in (None, _not_a_handle(), _matrix_magic_only()):
        assert L.spl_trisolve_solve_dev(operand, 0, 1, buf, 4, buf, 4, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_trisolve_solve_dev(operand, 9, -1, None, 0, None, 0, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_trisolve_solve(operand, 0, 1, buf, buf) == F.SPL_ERROR_invalid_handle
        assert L.spl_trisolve_info(operand, info) == F.SPL_ERROR_invalid_handle
        assert list(info) == [-7] * 8
    # free: NULL, a pointer to NULL, and a pointer to what is no object (nulled, nothing released)
    L.spl_trisolve_free(None)
    t = C.c_void_p(0)
    L.spl_trisolve_free(C.byref(t))
    assert not t.value
    foreign = _not_a_handle()
    t = C.c_void_p(C.addressof(foreign))
    L.spl_trisolve_free(C.byref(t))
    assert not t.value
    L.spl_trisolve_free(C.byref(t))
