"""The order in which spl_lobpcg_set_mass refuses its arguments (csrc/abi.hip), called raw through ctypes on an 8 x 8
Hermitian positive definite tridiagonal handle, real and complex, in the manner of tests/test_gpu_lobpcg_refusals.py: a
refused call breaks TWO rules where it can, the one whose status is expected and one further down the ladder of
include/sparse_linear_hip.h.  A solve while B has been freed is the caller's fault and is not tested."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_solver_refusals import DIM, HANDLE, N, OK, handle_of, tridiagonal, vp

pytestmark = pytest.mark.gpu

MATRIX = -8  # SPL_ERROR_invalid_matrix
BLOCK = 2


def info_of(L, solver):
    out = (C.c_int64 * 8)()
    assert L.spl_lobpcg_info(solver, out) == OK
    return list(out)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_set_mass_refuses_in_the_header_s_order(gpu, pkg, cplx):
    L = pkg._ffi.lib()
    A = handle_of(pkg, tridiagonal(N, cplx))
    B = handle_of(pkg, tridiagonal(N, cplx))
    small = handle_of(pkg, tridiagonal(N - 1, cplx))                      # the wrong size
    other = handle_of(pkg, tridiagonal(N, not cplx))                      # the other value kind
    skew = tridiagonal(N, cplx).tolil()
    skew[0, 1] = 0.5
    skew = handle_of(pkg, sp.csc_matrix(skew))                            # not Hermitian
    skew_small = tridiagonal(N - 1, cplx).tolil()
    skew_small[0, 1] = 0.5
    skew_small = handle_of(pkg, sp.csc_matrix(skew_small))               # not Hermitian AND of the wrong size
    wide = handle_of(pkg, sp.csc_matrix(np.ones((N, N + 1)) + (0j if cplx else 0.0)))
    # a row block; the library makes real ones only, so on a complex A it is refused for its value kind first
    real = tridiagonal(N, False)
    real.sort_indices()
    block = pkg.DeviceMatrix.from_csc(pkg.Matrix(N, N, real.indptr, real.indices, real.data), 0, 2)
    solver = vp()
    assert L.spl_lobpcg_create(A.handle, BLOCK, C.byref(solver)) == OK
    try:
        plain = info_of(L, solver)
        junk = C.create_string_buffer(256)
        ladder = [
            (A.handle, small.handle, HANDLE),      # L is a matrix, no solver: the handle before the size
            (None, skew.handle, HANDLE),
            (junk, B.handle, HANDLE),
            (solver, junk, HANDLE),                # B is no matrix handle
            (solver, solver, HANDLE),              # a solver object is no matrix
            (solver, skew_small.handle, DIM),      # the size before the values
            (solver, small.handle, DIM),
            (solver, wide.handle, DIM),
            (solver, other.handle, DIM),           # a real B on a complex A, and the other way round
            (solver, block.handle, DIM if cplx else MATRIX),  # a row block: N x N as a whole, but not whole
            (solver, skew.handle, MATRIX),
        ]
        for first, second, status in ladder:
            assert L.spl_lobpcg_set_mass(first, second) == status, (status,)
            assert info_of(L, solver) == plain  # a refused call changes nothing
        assert L.spl_lobpcg_set_mass(solver, B.handle) == OK
        with_mass = info_of(L, solver)
        vw = 2 if cplx else 1
        assert with_mass[2] == plain[2] | 32 and with_mass[3] == plain[3] + (3 * BLOCK + 1) * N * vw * 8
        assert L.spl_lobpcg_set_mass(solver, skew.handle) == MATRIX and info_of(L, solver) == with_mass  # B stays
        assert L.spl_lobpcg_set_mass(solver, B.handle) == OK and info_of(L, solver) == with_mass  # again: no second block
        assert L.spl_lobpcg_set_mass(solver, None) == OK and info_of(L, solver) == plain
        assert L.spl_lobpcg_set_mass(solver, None) == OK and info_of(L, solver) == plain
    finally:
        L.spl_lobpcg_free(C.byref(solver))
    assert L.spl_lobpcg_set_mass(solver, B.handle) == HANDLE  # the freed object
