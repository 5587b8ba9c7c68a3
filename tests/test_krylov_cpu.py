"""Preconditioned CG and BiCGSTAB on device handles (spl_vector_dot_dev, spl_krylov_*): what the calls answer before
the device is touched, and the yardstick of the GPU tests (tests/krylov_cases.py) checked on its own — the restated fold
against math.fsum, the restated drivers against the true residual.  What needs a GPU is in tests/test_gpu_krylov.py."""
import ctypes as C
import math

import numpy as np
import pytest

import krylov_cases as K

U53 = 2.0 ** -53
SYMBOLS = {"spl_vector_dot_dev": 6, "spl_krylov_create": 3, "spl_krylov_set_preconditioner": 4, "spl_krylov_solve_dev": 11,
           "spl_krylov_solve": 9, "spl_krylov_info": 2}


def _not_a_handle():
    return C.create_string_buffer(256)


def _matrix_magic_only(nrows_global=0, ncols=0, row0=0, nrows_local=0):
    """the magic word of a matrix handle ("SPLM") and its dimensions (magic, device, then nrows_global, ncols, row0,
    nrows_local as 64-bit words), zeros behind them"""
    buf = C.create_string_buffer(b"MLPS" + bytes(508))
    words = C.cast(buf, C.POINTER(C.c_int64))
    words[1], words[2], words[3], words[4] = nrows_global, ncols, row0, nrows_local
    return buf


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert L.spl_krylov_free.restype is None and len(L.spl_krylov_free.argtypes) == 1
    assert (pkg._ffi.SPL_KRYLOV_cg, pkg._ffi.SPL_KRYLOV_bicgstab) == (0, 1)


def test_the_python_surface_exists(pkg):
    S = pkg.sparse.KrylovSolver
    for name in ("solve", "solve_dev", "info", "free", "set_preconditioner"):
        assert callable(getattr(S, name)), name
    assert pkg.KrylovSolver is S and callable(pkg.DeviceMatrix.krylov)
    assert pkg.cg is pkg.sparse.cg and pkg.bicgstab is pkg.sparse.bicgstab and callable(pkg.vector_dot_dev)
    assert S.REASONS == K.REASONS and len(S.INFO_KEYS) == 8
    with pytest.raises(ValueError):
        S(pkg.DeviceMatrix(None), "gmres")
    with pytest.raises(pkg.SparseLinearError):
        pkg.DeviceMatrix(None).krylov("cg")


def test_create_refuses_in_the_documented_order(pkg):
    F = pkg._ffi
    L = F.lib()
    for operand in (None, _not_a_handle()):
        k = C.c_void_p(0x1234)  # not written: the operand is refused first
        assert L.spl_krylov_create(operand, 0, C.byref(k)) == F.SPL_ERROR_invalid_handle
        assert k.value == 0x1234
        assert L.spl_krylov_create(operand, 7, None) == F.SPL_ERROR_invalid_handle
    rect = _matrix_magic_only(3, 2, 0, 3)
    assert L.spl_krylov_create(rect, 0, None) == F.SPL_ERROR_argument_missing
    k = C.c_void_p(0x1234)
    assert L.spl_krylov_create(rect, 7, C.byref(k)) == F.SPL_ERROR_argument_missing and not k.value  # unknown method
    k = C.c_void_p(0x1234)
    assert L.spl_krylov_create(rect, 0, C.byref(k)) == F.SPL_ERROR_dimension_mismatch and not k.value
    block = _matrix_magic_only(4, 4, 2, 2)  # rows 2, 3 of a 4 x 4 matrix
    for method in (0, 1):
        k = C.c_void_p(0x1234)
        assert L.spl_krylov_create(block, method, C.byref(k)) == F.SPL_ERROR_invalid_matrix and not k.value


def test_without_a_gpu_create_answers_device(pkg):
    F = pkg._ffi
    if F.device_count() > 0:
        pytest.skip("a GPU is visible")
    whole = _matrix_magic_only(0, 0, 0, 0)
    k = C.c_void_p(0x1234)
    assert F.lib().spl_krylov_create(whole, 0, C.byref(k)) == F.SPL_ERROR_device and not k.value


def test_the_other_calls_refuse_what_is_no_solver(pkg):
    F = pkg._ffi
    L = F.lib()
    result = (C.c_int64 * 4)(-7, -7, -7, -7)
    info = (C.c_int64 * 8)(*([-7] * 8))
    for operand in (None, _not_a_handle(), _matrix_magic_only()):
        assert L.spl_krylov_set_preconditioner(operand, None, None, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_krylov_solve_dev(operand, None, None, 0, 1e-8, 0.0, 10, 0, result, None, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_krylov_solve(operand, None, None, 0, 1e-8, 0.0, 10, result, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_krylov_info(operand, info) == F.SPL_ERROR_invalid_handle
        assert list(result) == [-7] * 4 and list(info) == [-7] * 8
    L.spl_krylov_free(None)
    p = C.c_void_p(0)
    L.spl_krylov_free(C.byref(p))
    foreign = _not_a_handle()
    p = C.c_void_p(C.addressof(foreign))
    L.spl_krylov_free(C.byref(p))
    assert not p.value
    L.spl_krylov_free(C.byref(p))


def test_vector_dot_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    buf = C.create_string_buffer(64)
    at = (C.addressof(buf) + 15) & ~15
    assert L.spl_vector_dot_dev(-1, 1, at, at, at, None) == F.SPL_ERROR_n_nonpositive
    for width in (0, 3):
        assert L.spl_vector_dot_dev(4, width, at, at, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dot_dev(4, 1, None, at, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dot_dev(4, 1, at, None, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dot_dev(0, 1, None, None, None, None) == F.SPL_ERROR_argument_missing  # d_out is always needed
    assert L.spl_vector_dot_dev(4, 1, at + 4, at, at, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_dot_dev(4, 2, at + 8, at, at, None) == F.SPL_ERROR_argument_missing  # a pair is 16 bytes
    assert L.spl_vector_dot_dev(4, 2, at, at, at + 8, None) == F.SPL_ERROR_argument_missing


# ---- the restated fold -------------------------------------------------------------------------------------------------
SIZES = (0, 1, 255, 256, 257, 4095, 4096, 4097, 8229, 20005)


def fold_bound(products):
    """(ceil(len / 256) + 8 + levels 12) 2^-53 sum |a_i b_i|: a lane adds ceil(len / 256) values at most on the first
    level, the tree has 8 steps, and every further level adds 16 + 8 < 2 * 12 operations to a path"""
    n = len(products)
    return (-(-n // 256) + 8 + K.fold_levels(n) * 12) * U53 * math.fsum(np.abs(products).tolist())


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n", SIZES)
def test_restated_fold_against_fsum(n, cplx):
    a, b = K.dot_inputs(n, cplx)
    planes = K.arithmetic(cplx).products(a, b)
    got = K.dot(a, b)
    parts = (got.real, got.imag) if cplx else (got,)
    for plane, value in zip(planes, parts):
        want = math.fsum(plane.tolist())
        assert abs(value - want) <= fold_bound(plane), (n, abs(value - want), fold_bound(plane))
    if n >= 255:
        # the inputs cancel: the sum is far below the sum of the magnitudes
        assert abs(math.fsum(planes[0].tolist())) < 0.5 * math.fsum(np.abs(planes[0]).tolist())
    if n == 0:
        assert parts[0] == 0.0 and math.copysign(1.0, parts[0]) == 1.0


def test_restated_fold_is_the_lane_order():
    """one chunk by hand: lane t adds t, t + 256, ... from +0.0, then the tree"""
    v = np.random.default_rng(5).uniform(-1, 1, 700)
    lanes = [0.0] * 256
    for t in range(256):
        for i in range(t, 700, 256):
            lanes[t] = lanes[t] + float(v[i])
    h = 128
    while h >= 1:
        for t in range(h):
            lanes[t] = lanes[t] + lanes[t + h]
        h //= 2
    assert K.fold(v) == lanes[0]
    # two levels: the partials of three chunks are folded as a vector of three
    w = np.random.default_rng(6).uniform(-1, 1, 8229)
    partials = [K.fold(w[:4096]), K.fold(w[4096:8192]), K.fold(w[8192:])]
    assert K.fold(w) == K.fold(np.array(partials))
    assert K.fold(np.array(partials)) == (partials[0] + partials[2]) + partials[1]  # lanes 0 and 2 meet at h = 2


# ---- the restated drivers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.PRECONDITIONERS, ids=lambda k: str(k))
@pytest.mark.parametrize("method,name", K.CASES)
def test_restated_drivers_converge_to_the_true_solution(method, name, kind):
    out = K.reference(method, name, kind)
    assert out.reason == 0 and 0 < out.iterations < 2000, (out.reason, out.iterations)
    assert len(out.history) == out.iterations + 1
    b = K.rhs(name)
    assert out.history[-1] <= K.RTOL * np.linalg.norm(b) * (1 + 1e-12)
    true = K.true_relative_residual(K.matrix(name), out.x, b)
    assert true <= 10 * K.RTOL, true


@pytest.mark.parametrize("method,name", K.CASES)
def test_ilu0_needs_fewer_iterations(method, name):
    assert K.reference(method, name, "ilu0").iterations < K.reference(method, name, None).iterations


def test_restated_start_vector_and_max_iter():
    for method, name in (("cg", "poisson"), ("bicgstab", "shifted")):
        out = K.reference(method, name, "jacobi", start=True)
        assert out.reason == 0
        assert K.true_relative_residual(K.matrix(name), out.x, K.rhs(name)) <= 10 * K.RTOL
        three = K.reference(method, name, None, max_iter=3)
        assert (three.iterations, three.reason, len(three.history)) == (3, 1, 4)
        assert K.bits_equal(three.history, K.reference(method, name, None).history[:4])


def test_restated_endings():
    S2 = np.array([[1.0, 1.0], [1.0, 1.0]])
    import scipy.sparse as sp
    out = K.cg(sp.csr_matrix(S2), np.array([1.0, 0.0]), max_iter=50)
    assert out.reason in (1, 2)
    out = K.bicgstab(sp.csr_matrix(S2), np.array([1.0, 0.0]), max_iter=50)
    assert out.reason in (1, 2)
    minus = sp.csr_matrix(-np.eye(5))
    out = K.cg(minus, np.arange(1.0, 6.0))
    assert out.reason == 0 and np.allclose(out.x, -np.arange(1.0, 6.0))
    out = K.cg(minus, np.zeros(5))
    assert (out.iterations, out.reason) == (0, 0) and not out.x.any()
    bad = np.arange(1.0, 6.0)
    bad[2] = float("nan")
    assert K.cg(minus, bad).reason == 3 and K.bicgstab(minus, bad).reason == 3


def test_quality_case_is_shown_for_the_restatement():
    """poisson3d(30), ILU(0)-PCG, rtol 1e-10: the true residual and the iteration count the GPU test asks for"""
    S, b = K.matrix("poisson3d"), K.rhs("poisson3d")
    pre = K.reference("cg", "poisson3d", "ilu0", rtol=1e-10)
    plain = K.reference("cg", "poisson3d", None, rtol=1e-10)
    assert pre.reason == 0 and plain.reason == 0
    assert K.true_relative_residual(S, pre.x, b) <= 10 * 1e-10
    assert pre.iterations < plain.iterations
