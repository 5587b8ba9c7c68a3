"""Restarted GMRES on device handles (spl_vector_dots_dev, spl_gmres_*): what the calls answer before the device is
touched, and the yardstick of the GPU tests (tests/gmres_cases.py) checked on its own — the restated solver against the
true residual and numpy's orthogonality.  What needs a GPU is in tests/test_gpu_gmres.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import gmres_cases as GK
import krylov_cases as K

SYMBOLS = {"spl_vector_dots_dev": 8, "spl_gmres_create": 3, "spl_gmres_set_preconditioner": 4,
           "spl_gmres_set_preconditioner_amg": 2, "spl_gmres_solve_dev": 12, "spl_gmres_solve": 10, "spl_gmres_info": 2}


def _not_a_handle():
    return C.create_string_buffer(256)


def _matrix_magic_only(nrows_global=0, ncols=0, row0=0, nrows_local=0):
    """the magic word of a matrix handle ("SPLM") and its dimensions (magic, device, then nrows_global, ncols, row0,
    nrows_local as 64-bit words), zeros behind them"""
    buf = C.create_string_buffer(b"MLPS" + bytes(508))
    words = C.cast(buf, C.POINTER(C.c_int64))
    words[1], words[2], words[3], words[4] = nrows_global, ncols, row0, nrows_local
    return buf


def _gmres_magic_only(n=0, width=1):
    """the magic word of a GMRES object ("SPLG"), then device, value width and restart as 32-bit words and n as a 64-bit
    one, zeros behind them"""
    buf = C.create_string_buffer(b"GLPS" + bytes(1020))
    words32 = C.cast(buf, C.POINTER(C.c_int32))
    words32[2], words32[3] = width, 5
    C.cast(buf, C.POINTER(C.c_int64))[2] = n
    return buf


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert L.spl_gmres_free.restype is None and len(L.spl_gmres_free.argtypes) == 1


def test_the_python_surface_exists(pkg):
    S = pkg.sparse.GMRESSolver
    for name in ("solve", "solve_dev", "info", "free", "set_preconditioner"):
        assert callable(getattr(S, name)), name
    assert pkg.GMRESSolver is S and callable(pkg.DeviceMatrix.gmres)
    assert pkg.gmres is pkg.sparse.gmres and pkg.vector_dots_dev is pkg.sparse.vector_dots_dev
    assert S.REASONS == GK.REASONS and len(S.INFO_KEYS) == 8 and len(S.RESULT_KEYS) == 6
    for restart in (0, 129):
        with pytest.raises(ValueError):
            S(pkg.DeviceMatrix(None), restart)
    with pytest.raises(pkg.SparseLinearError):
        pkg.DeviceMatrix(None).gmres(30)
    # GMRES is an object of its own: the CG / BiCGSTAB object keeps refusing the name, and keeps what it exposes
    KS = pkg.sparse.KrylovSolver
    with pytest.raises(ValueError):
        KS(pkg.DeviceMatrix(None), "gmres")
    assert sorted(KS.METHODS) == ["bicgstab", "cg"] and len(KS.INFO_KEYS) == 8 and KS.REASONS == S.REASONS
    for name in ("solve", "solve_dev", "info", "free", "set_preconditioner", "handle", "_free", "_result", "_maxiter",
                 "_diagonal"):
        assert hasattr(KS, name), name


def test_create_refuses_in_the_documented_order(pkg):
    F = pkg._ffi
    L = F.lib()
    for operand in (None, _not_a_handle()):
        g = C.c_void_p(0x1234)  # not written: the operand is refused first
        assert L.spl_gmres_create(operand, 30, C.byref(g)) == F.SPL_ERROR_invalid_handle
        assert g.value == 0x1234
        assert L.spl_gmres_create(operand, 0, None) == F.SPL_ERROR_invalid_handle
    rect = _matrix_magic_only(3, 2, 0, 3)
    assert L.spl_gmres_create(rect, 30, None) == F.SPL_ERROR_argument_missing
    for restart in (0, -1, 129):  # where "unknown method" comes in spl_krylov_create: before the shape is looked at
        g = C.c_void_p(0x1234)
        assert L.spl_gmres_create(rect, restart, C.byref(g)) == F.SPL_ERROR_argument_missing and not g.value
    for restart in (1, 128):
        g = C.c_void_p(0x1234)
        assert L.spl_gmres_create(rect, restart, C.byref(g)) == F.SPL_ERROR_dimension_mismatch and not g.value
    block = _matrix_magic_only(4, 4, 2, 2)  # rows 2, 3 of a 4 x 4 matrix
    g = C.c_void_p(0x1234)
    assert L.spl_gmres_create(block, 30, C.byref(g)) == F.SPL_ERROR_invalid_matrix and not g.value  # restart > n is allowed
    # the CG / BiCGSTAB object still knows two methods
    k = C.c_void_p(0x1234)
    assert L.spl_krylov_create(rect, 2, C.byref(k)) == F.SPL_ERROR_argument_missing and not k.value


def test_the_other_calls_refuse_what_is_no_solver(pkg):
    F = pkg._ffi
    L = F.lib()
    result = (C.c_int64 * 6)(*([-7] * 6))
    residual = (C.c_double * 2)(-7.0, -7.0)
    info = (C.c_int64 * 8)(*([-7] * 8))
    for operand in (None, _not_a_handle(), _matrix_magic_only()):
        assert L.spl_gmres_set_preconditioner(operand, None, None, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_gmres_set_preconditioner_amg(operand, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_gmres_solve_dev(operand, None, None, 0, 1e-8, 0.0, 10, 0, result, None, residual, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_gmres_solve(operand, None, None, 0, 1e-8, 0.0, 10, result, None, residual) == F.SPL_ERROR_invalid_handle
        assert L.spl_gmres_info(operand, info) == F.SPL_ERROR_invalid_handle
        assert list(result) == [-7] * 6 and list(info) == [-7] * 8 and list(residual) == [-7.0, -7.0]
    L.spl_gmres_free(None)
    p = C.c_void_p(0)
    L.spl_gmres_free(C.byref(p))
    foreign = _not_a_handle()
    p = C.c_void_p(C.addressof(foreign))
    L.spl_gmres_free(C.byref(p))
    assert not p.value
    L.spl_gmres_free(C.byref(p))


def test_solve_refuses_in_the_documented_order(pkg):
    """on an object that is only its magic word and its dimensions: nothing here reaches the device"""
    F = pkg._ffi
    L = F.lib()
    G = _gmres_magic_only(n=8, width=2)
    result = (C.c_int64 * 6)(*([-7] * 6))
    residual = (C.c_double * 2)(-7.0, -7.0)
    hist = (C.c_double * 4)()
    buf = C.create_string_buffer(512)
    b = (C.addressof(buf) + 15) & ~15
    x = b + 256

    def dev(b_ptr, x_ptr, rtol=1e-8, atol=0.0, max_iter=10, every=0, res=result, history=None, rsd=residual):
        return L.spl_gmres_solve_dev(G, b_ptr, x_ptr, 0, rtol, atol, max_iter, every, res, history, rsd, None)

    assert dev(None, None, res=None, max_iter=-1) == F.SPL_ERROR_argument_missing  # result before max_iter
    assert dev(None, None, rsd=None, max_iter=-1) == F.SPL_ERROR_argument_missing  # residual where result is
    assert dev(None, None, max_iter=-1, rtol=-1.0) == F.SPL_ERROR_n_nonpositive      # max_iter before the tolerances
    assert dev(None, None, rtol=-1.0) == F.SPL_ERROR_argument_missing
    assert dev(None, None, atol=float("nan")) == F.SPL_ERROR_argument_missing
    assert dev(None, None, every=-1) == F.SPL_ERROR_argument_missing
    assert dev(None, None, max_iter=2 ** 31, history=hist) == F.SPL_ERROR_index_overflow  # before the vectors
    assert dev(None, x) == F.SPL_ERROR_argument_missing
    assert dev(b, None) == F.SPL_ERROR_argument_missing
    assert dev(b, b) == F.SPL_ERROR_argument_missing
    assert dev(b + 8, x) == F.SPL_ERROR_argument_missing  # a pair is 16 bytes
    assert dev(b, x + 8) == F.SPL_ERROR_argument_missing
    assert L.spl_gmres_solve(G, None, None, 0, 1e-8, 0.0, 10, None, None, residual) == F.SPL_ERROR_argument_missing
    assert L.spl_gmres_solve(G, None, None, 0, 1e-8, 0.0, 10, result, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_gmres_solve(G, None, None, 0, 1e-8, 0.0, -1, result, None, residual) == F.SPL_ERROR_n_nonpositive
    assert L.spl_gmres_solve(G, None, None, 0, 1e-8, 0.0, 10, result, None, residual) == F.SPL_ERROR_argument_missing
    assert list(result) == [-7] * 6 and list(residual) == [-7.0, -7.0]
    # an empty system is answered before the vectors are looked at
    empty = _gmres_magic_only(n=0)
    assert L.spl_gmres_solve_dev(empty, None, None, 0, 1e-8, 0.0, 3, 0, result, hist, residual, None) == 0
    assert list(result) == [0] * 6 and list(residual) == [0.0, 0.0] and hist[0] == 0.0
    # the preconditioner calls look at the parts before anything else
    assert L.spl_gmres_set_preconditioner(G, _not_a_handle(), None, None) == F.SPL_ERROR_invalid_handle
    assert L.spl_gmres_set_preconditioner(G, None, C.c_void_p(b + 8), None) == F.SPL_ERROR_argument_missing
    assert L.spl_gmres_set_preconditioner_amg(G, _not_a_handle()) == F.SPL_ERROR_invalid_handle


def test_vector_dots_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    buf = C.create_string_buffer(256)
    at = (C.addressof(buf) + 15) & ~15
    assert L.spl_vector_dots_dev(-1, 0, 0, None, -5, None, None, None) == F.SPL_ERROR_n_nonpositive
    for width in (0, 3):
        assert L.spl_vector_dots_dev(4, width, 0, None, 0, None, None, None) == F.SPL_ERROR_argument_missing
    for k in (0, -1, 129):
        assert L.spl_vector_dots_dev(4, 1, k, at, 4, at, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dots_dev(4, 1, 2, at, 3, at, at, None) == F.SPL_ERROR_argument_missing  # ldv < n
    assert L.spl_vector_dots_dev(4, 1, 2, None, 4, at, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dots_dev(4, 1, 2, at, 4, None, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dots_dev(4, 1, 2, at, 4, at, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dots_dev(0, 1, 2, None, 0, None, None, None) == F.SPL_ERROR_argument_missing  # d_out is always needed
    assert L.spl_vector_dots_dev(4, 1, 2, at + 4, 4, at, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dots_dev(4, 2, 2, at + 8, 4, at, at, None) == F.SPL_ERROR_argument_missing  # a pair is 16 bytes
    assert L.spl_vector_dots_dev(4, 2, 2, at, 4, at + 8, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dots_dev(4, 2, 2, at, 4, at, at + 8, None) == F.SPL_ERROR_argument_missing


# ---- the restatement, checked on its own -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,restart", GK.SELF_CHECKED, ids=lambda v: str(v))
def test_restated_gmres_converges_to_the_true_solution(name, kind, restart):
    out = GK.reference(name, kind, restart, keep_basis=True)
    b = K.rhs(name)
    true = K.true_relative_residual(K.matrix(name), out.x, b)
    print("%s %s restart %d: %d iterations in %d cycles, reason %d, true relative residual %.3e"
          % (name, kind, restart, out.iterations, out.cycles, out.reason, true))
    assert out.reason == 0
    assert true <= 1e-8 * (1 + 1e-6), true  # the margin: scipy's product sums in another order than the restated one
    assert len(out.history) == out.iterations + 1 and 0 < out.iterations < 2000
    assert -(-out.iterations // restart) <= out.cycles <= out.iterations  # a cycle does at least a step, at most `restart`
    assert out.spmvs == out.iterations + out.cycles and out.applications == (0 if kind is None else out.spmvs)
    assert out.residual[0] <= 1e-8 * np.linalg.norm(b) * (1 + 1e-12)  # what reason 0 was decided on
    V = out.basis
    assert V.shape[0] == len(b) and 1 <= V.shape[1] <= restart
    gram = V.conj().T @ V
    assert np.max(np.abs(gram - np.eye(V.shape[1]))) <= 1e-12


def test_restated_endings():
    two = sp.csr_matrix(2.0 * np.eye(5000))
    b = np.zeros(5000)
    b[:4096] = 1.0  # |b| = 64: v_0 and <v_0, A v_0> are exact, so w vanishes exactly
    out = GK.gmres(two, b)
    assert (out.iterations, out.reason, out.cycles) == (1, 0, 1) and out.history[1] == 0.0
    assert np.array_equal(out.x, 0.5 * b) and out.residual.tolist() == [0.0, 0.0]
    zeros = sp.csr_matrix((np.zeros(5), np.arange(5), np.arange(6)), shape=(5, 5))
    start = np.arange(1.0, 6.0)
    out = GK.gmres(zeros, np.ones(5), x0=start)
    assert (out.iterations, out.reason) == (0, 2) and np.array_equal(out.x, start)
    bad = np.eye(5)
    bad[1, 2] = np.inf
    out = GK.gmres(sp.csr_matrix(bad), np.ones(5))
    assert (out.iterations, out.reason) == (0, 3) and not out.x.any()
    nan = np.ones(5)
    nan[3] = np.nan
    out = GK.gmres(two[:5, :5], nan)
    assert (out.iterations, out.reason, out.cycles) == (0, 3, 0)
    out = GK.gmres(two[:5, :5], np.zeros(5))
    assert (out.iterations, out.reason, out.cycles) == (0, 0, 0) and not out.x.any() and out.history.tolist() == [0.0]
    small = sp.csr_matrix(np.array([[4.0, 1.0, 0.0], [2.0, 5.0, 1.0], [0.0, -1.0, 3.0]]))
    out = GK.gmres(small, np.array([1.0, 2.0, 3.0]), restart=30)
    assert out.reason == 0 and out.iterations <= 4
    assert K.true_relative_residual(small, out.x, np.array([1.0, 2.0, 3.0])) <= 1e-8 * (1 + 1e-6)


def test_restated_max_iter_and_start():
    name = "unsym"
    whole = GK.reference(name, None, 30)
    cut = GK.reference(name, None, 30, max_iter=45)
    assert (cut.iterations, cut.reason) == (45, 1) and cut.iterations % 30 != 0  # in mid cycle
    assert K.bits_equal(cut.history[:31], whole.history[:31])
    started = GK.reference(name, "jacobi", 5, start=True)
    assert started.reason == 0 and not K.bits_equal(started.history[:1], GK.reference(name, "jacobi", 5).history[:1])
    assert started.spmvs == started.iterations + started.cycles + 1  # the first residual needs a product too
