"""ILU(0) on device handles (spl_ilu0_analyze, _factor, _info, _free, spl_matrix_ilu0): what the calls answer before the
device is touched, and the yardstick of the GPU tests checked against an independent dense LU.  Argument checks come
first, so these hold with or without a GPU; what needs a real handle and a real plan is in tests/test_gpu_ilu0.py."""
import ctypes as C

import numpy as np
import pytest

import ilu0_cases as K

SYMBOLS = {"spl_ilu0_analyze": 2, "spl_ilu0_factor": 3, "spl_ilu0_info": 2, "spl_matrix_ilu0": 2}


def _not_a_handle():
    """memory that is readable where a magic word would be, and holds none"""
    return C.create_string_buffer(256)


def _matrix_magic_only():
    """the first four bytes of a matrix handle ("SPLM" as a little-endian word), zeros behind them: a 0 x 0 matrix
    without row pointers to whoever reads on"""
    return C.create_string_buffer(b"MLPS" + bytes(508))


def _plan_magic_only():
    """the magic word of an ILU(0) plan ("SPLI") and zeros: n = 0, nnz = 0, device 0, no arrays"""
    return C.create_string_buffer(b"ILPS" + bytes(1020))


def test_the_five_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes and len(fn.argtypes) == nargs, name
    free = L.spl_ilu0_free
    assert free.restype is None and len(free.argtypes) == 1


def test_the_python_surface_exists(pkg):
    assert callable(pkg.DeviceMatrix.ilu0)
    I = pkg.sparse.ILU0
    for name in ("info", "refactor", "solve", "apply_dev", "free"):
        assert callable(getattr(I, name)), name
    assert I.INFO_KEYS[:4] == ("n", "nnz", "levels", "launches") and len(I.INFO_KEYS) == 8
    assert callable(pkg.sparse.ilu0) and pkg.ilu0 is pkg.sparse.ilu0 and pkg.ILU0 is I
    # an object that holds nothing refuses before any handle is looked at
    with pytest.raises(pkg.SparseLinearError):
        pkg.DeviceMatrix(None).ilu0()


def test_analyze_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    for operand in (None, _not_a_handle(), _plan_magic_only()):
        p = C.c_void_p(0x1234)  # not written: the operand is refused first
        assert L.spl_ilu0_analyze(operand, C.byref(p)) == F.SPL_ERROR_invalid_handle
        assert p.value == 0x1234
        assert L.spl_ilu0_analyze(operand, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_matrix_ilu0(operand, C.byref(p)) == F.SPL_ERROR_invalid_handle
        assert p.value == 0x1234
    fake = _matrix_magic_only()
    assert L.spl_ilu0_analyze(fake, None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_ilu0(fake, None) == F.SPL_ERROR_argument_missing
    # a square "handle" without 32-bit row pointers; *P is cleared once the output is known to exist
    for call in (L.spl_ilu0_analyze, L.spl_matrix_ilu0):
        p = C.c_void_p(0x1234)
        assert call(fake, C.byref(p)) == F.SPL_ERROR_invalid_matrix
        assert not p.value
    # not square: the dimensions are looked at before the row pointers (nrows_global, ncols follow magic and device)
    rect = _matrix_magic_only()
    C.cast(rect, C.POINTER(C.c_int64))[1] = 3  # nrows_global
    p = C.c_void_p(0x1234)
    assert L.spl_ilu0_analyze(rect, C.byref(p)) == F.SPL_ERROR_dimension_mismatch
    assert not p.value


def test_factor_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    plan, matrix = _plan_magic_only(), _matrix_magic_only()
    for p, h in ((None, matrix), (_not_a_handle(), matrix), (matrix, matrix), (plan, None), (plan, _not_a_handle()),
                 (plan, plan)):
        f = C.c_void_p(0x1234)
        assert L.spl_ilu0_factor(p, h, C.byref(f)) == F.SPL_ERROR_invalid_handle
        assert f.value == 0x1234
        assert L.spl_ilu0_factor(p, h, None) == F.SPL_ERROR_invalid_handle
    assert L.spl_ilu0_factor(plan, matrix, None) == F.SPL_ERROR_argument_missing
    f = C.c_void_p(0x1234)
    assert L.spl_ilu0_factor(plan, matrix, C.byref(f)) == F.SPL_ERROR_invalid_matrix  # no 32-bit row pointers
    assert not f.value


def test_info_and_free_refuse_what_is_no_plan(pkg):
    F = pkg._ffi
    L = F.lib()
    info = (C.c_int64 * 8)(*([-7] * 8))
    for operand in (None, _not_a_handle(), _matrix_magic_only()):  # a matrix handle's magic is not a plan's
        assert L.spl_ilu0_info(operand, info) == F.SPL_ERROR_invalid_handle
        assert list(info) == [-7] * 8
    plan = _plan_magic_only()
    assert L.spl_ilu0_info(plan, None) == F.SPL_ERROR_argument_missing
    assert L.spl_ilu0_info(plan, info) == F.SPL_OK and list(info) == [0] * 8
    # free: NULL, a pointer to NULL, and a pointer to what is no plan (nulled, nothing released)
    L.spl_ilu0_free(None)
    p = C.c_void_p(0)
    L.spl_ilu0_free(C.byref(p))
    assert not p.value
    for foreign in (_not_a_handle(), _matrix_magic_only()):
        p = C.c_void_p(C.addressof(foreign))
        L.spl_ilu0_free(C.byref(p))
        assert not p.value
        L.spl_ilu0_free(C.byref(p))


# ---- the yardstick itself ----------------------------------------------------------------------------------------------
def dense_lu_without_pivoting(A):
    """Doolittle's elimination on a dense array, column by column of the trailing block (the KIJ order, numpy's
    arithmetic): independent of the restatement's loop order and of its look-ups"""
    A = np.array(A)
    n = A.shape[0]
    for k in range(n - 1):
        A[k + 1:, k] = A[k + 1:, k] / A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return A


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name,size", [("tridiagonal", 200), ("dense70", 70), ("arrow", 100)])
def test_restatement_is_the_lu_on_patterns_without_fill(name, size, cplx):
    """where elimination creates no fill, ILU(0) is the LU factorisation: every entry agrees with the dense one to
    1e-13 RELATIVE to that entry.  (Each entry sees the same updates in the same order of k in both computations; only
    numpy's complex product may round differently.)  The backward-error scale beside it is the weaker, derived check:
    both differ from the exact factors by at most gamma_n (|L||U|)_ij, n <= 200 steps, 200 * 2^-53 = 2.2e-14 each"""
    S = K.matrix(name, cplx, size)
    got = K.serial_ilu0(S)
    want = dense_lu_without_pivoting(S.toarray())
    n = S.shape[0]
    assert np.count_nonzero(want) == S.nnz  # no fill indeed
    scale = np.abs(np.tril(want, -1) + np.eye(n)) @ np.abs(np.triu(want))
    rows = np.repeat(np.arange(n), np.diff(S.indptr))
    err = np.abs(got - want[rows, S.indices])
    entry = np.abs(want[rows, S.indices])
    assert np.all(err <= 1e-13 * entry), float(np.max(err / entry))
    assert np.all(err <= 1e-13 * scale[rows, S.indices]), float(np.max(err / scale[rows, S.indices]))


def test_committed_cases_are_finite_and_cover_every_group_width():
    for name in K.NAMES:
        for cplx in (False, True):
            out = K.reference(name, cplx)  # asserts finiteness and the size of the restatement
            assert len(out) == K.matrix(name, cplx).nnz
    R = K.matrix("random", False)
    lens = np.diff(R.indptr)
    assert lens.min() == 1 and lens.max() == 300 and R.shape[0] == 600
    assert K.groups_of_rows(R) == {1, 2, 4, 8, 16, 32, 64}
    assert K.levels_of(R) == list(range(600))  # one row per level: with every level wide, G follows each row's length
    for cplx in (False, True):
        both, zero, good = K.pivots_cases(cplx)
        assert not np.all(np.isfinite(K.serial_ilu0(both).view(np.float64)))
        assert not np.all(np.isfinite(K.serial_ilu0(zero).view(np.float64)))
        assert np.all(np.isfinite(K.serial_ilu0(good).view(np.float64)))
