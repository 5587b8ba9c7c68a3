"""The restatement of tests/lobpcg_cases.py checked on its own, without a GPU, against numpy: every converging case
reaches reason 0 inside its max_iter, the values are the wanted ones within the Hermitian residual bound, the copies of a
multiple eigenvalue are independent, and the complex Jacobi reproduces eigvalsh.  Also the symbols and the Python
surface, and what the calls answer before the device is touched.

Measured |X^H X - I| (max entry) of the returned blocks: poisson12 smallest 4.4e-16, phased12 2.2e-16, poisson12 largest
2.2e-16, five 4.4e-16, two 1.1e-16, grid70 (stopped at 3 iterations) 2.2e-16, poisson8 with Jacobi 3.3e-16, symmetric
Gauss-Seidel 2.2e-16, ILU(0) 2.2e-16.  With X' rotated and never orthonormalised again, as the method was first written,
the figures were 1.2e-13, 1.3e-13, 7.0e-14, 4.4e-16, 4.4e-16, 3.8e-15, 8.3e-14, 3.3e-14 and 3.1e-14, growing with the
iterations, and the smallest value of poisson12 missed the bound below (1.89e-14 against 1.78e-14, theta biased upwards by
the loss): that is why every close settles X' again."""
import ctypes as C

import numpy as np
import pytest

import lobpcg_cases as LK

EPS = 2.0 ** -53
SYMBOLS = {"spl_lobpcg_create": 3, "spl_lobpcg_set_preconditioner": 4, "spl_lobpcg_set_preconditioner_amg": 2,
           "spl_lobpcg_solve_dev": 15, "spl_lobpcg_solve": 14, "spl_lobpcg_info": 2}
HANDLE, MISSING = -3, -5


def check_against_numpy(out, S, which, nev):
    """the sorted theta against the sorted wanted eigvalsh values within res_i / |x_i| + 8 2^-53 |A|_1, and the smallest
    singular value of X at least 0.99: the copies are independent"""
    exact = np.linalg.eigvalsh(S.toarray())
    wanted = np.sort(exact[::-1][:nev] if which == LK.LARGEST else exact[:nev])
    got = np.sort(out.values)
    by_value = np.argsort(out.values, kind="stable")
    floor = 8.0 * EPS * LK.norm_one(S)
    for k in range(nev):
        i = by_value[k]
        bound = out.residuals[i] / np.linalg.norm(out.vectors[:, i]) + floor
        print("theta %.17g  wanted %.17g  |difference| %.3e  bound %.3e" % (got[k], wanted[k], abs(got[k] - wanted[k]), bound))
        assert abs(got[k] - wanted[k]) <= bound
    smallest = np.linalg.svd(out.vectors, compute_uv=False).min()
    print("sigma_min(X) %.15f  |X^H X - I| %.3e" % (smallest, np.abs(out.vectors.conj().T @ out.vectors - np.eye(nev)).max()))
    assert smallest >= 0.99


@pytest.mark.parametrize("case", [c for c in LK.CASES if c[0] != "grid70"], ids=lambda c: "-".join(str(v) for v in c))
def test_cases_converge_to_numpy_s_extreme_values(case):
    name, block, nev, which, tol, max_iter = case
    out = LK.reference(*case)
    assert out.reason == 0 and out.pairs == nev and out.iterations <= max_iter
    assert len(out.history) == out.iterations + 1 and out.sweeps <= LK.MAX_SWEEPS
    assert out.history[-1] <= tol * np.abs(out.values).max()  # the largest residual norm of the last check
    assert out.syncs == 2 + 2 * out.iterations + 2  # the start, its close; two per iteration; the last check, the finish
    check_against_numpy(out, LK.matrix(name), which, nev)


def test_both_copies_of_the_double_eigenvalue_are_returned():
    for name in ("poisson12", "phased12"):
        out = LK.reference(name, 6, 4, LK.SMALLEST, 1e-9, 200)
        exact = np.linalg.eigvalsh(LK.matrix(name).toarray())
        assert abs(exact[1] - exact[2]) < 1e-12 < exact[3] - exact[2]  # lambda_2 is double
        theta = np.sort(out.values)
        assert abs(theta[1] - exact[1]) < 1e-9 and abs(theta[2] - exact[2]) < 1e-9


@pytest.mark.parametrize("kind", ["jacobi", "sgs", "ilu0"])
def test_preconditioned_cases_converge(kind):
    block, nev, tol, max_iter = [c for c in LK.PRECONDITIONED if c[0] == kind][0][1:]
    out = LK.reference("poisson8", block, nev, LK.SMALLEST, tol, max_iter, kind)
    assert out.reason == 0 and out.applications == block * out.iterations
    check_against_numpy(out, LK.matrix("poisson8"), LK.SMALLEST, nev)


def test_outcomes_of_the_header():
    # n = 5, block = 2: 3 block > n, so a column must drop
    out = LK.reference("five", 2, 2, LK.SMALLEST, 1e-10, 50)
    assert out.reason == 0 and out.dropped >= 1
    # a diagonal matrix and unit vectors: R = 0, converged at iteration 0, nothing multiplied but the start and the finish
    D = LK.matrix("diagonal")
    out = LK.lobpcg(D, np.eye(8)[:, :3], 2, LK.SMALLEST, 1e-10, 0.0, 50)
    assert out.result == [0, 0, 3 + 2, 2, 0, 0, 0, 4] and list(out.values) == [1.0, 2.0] and list(out.residuals) == [0.0, 0.0]
    # a repeated column: reason 2; a NaN: reason 3; no pairs
    X = LK.start_block(8, 3)
    X[:, 2] = X[:, 0]
    out = LK.lobpcg(D, X, 2)
    assert out.result == [2, 0, 0, 0, 0, 0, 0, 1] and out.vectors.shape == (8, 0)
    X = LK.start_block(8, 3)
    X[4, 1] = np.nan
    assert LK.lobpcg(D, X, 2).result == [3, 0, 0, 0, 0, 0, 0, 1]
    # max_iter
    out = LK.reference("grid70", 4, 2, LK.SMALLEST, 1e-9, 3)
    assert out.reason == 1 and out.iterations == 3 and out.pairs == 2 and len(out.history) == 4
    # largest
    out = LK.reference("poisson12", 4, 2, LK.LARGEST, 1e-9, 200)
    assert out.values[0] >= out.values[1] > 7.0


@pytest.mark.parametrize("m", [1, 2, 3, 17, 60])
def test_complex_jacobi_reproduces_eigvalsh(m):
    rng = np.random.default_rng(m)
    B = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
    T = (B + B.conj().T) / 2.0
    Tr = [list(map(float, row)) for row in T.real]
    Ti = [list(map(float, row)) for row in T.imag]
    theta, Yr, Yi, sweeps = LK.jacobi_hermitian(Tr, Ti)
    Y = np.array(Yr) + 1j * np.array(Yi)
    scale = 8.0 * m * EPS * np.linalg.norm(T)
    print("order %d  sweeps %d  |theta - eigvalsh| %.3e  |Y^H Y - I| %.3e  scale %.3e"
          % (m, sweeps, np.abs(np.sort(theta) - np.linalg.eigvalsh(T)).max(), np.abs(Y.conj().T @ Y - np.eye(m)).max(), scale))
    assert sweeps <= 12
    assert np.abs(np.sort(theta) - np.linalg.eigvalsh(T)).max() <= scale
    assert np.abs(Y.conj().T @ Y - np.eye(m)).max() <= scale
    assert np.abs(Y @ np.diag(theta) @ Y.conj().T - T).max() <= scale


def test_the_symbols_and_the_python_surface(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes and len(fn.argtypes) == nargs, name
    assert L.spl_lobpcg_free.restype is None
    assert pkg.lobpcg is pkg.sparse.lobpcg and pkg.LOBPCGSolver is pkg.sparse.LOBPCGSolver
    assert callable(pkg.DeviceMatrix.lobpcg)
    assert pkg.LOBPCGSolver.REASONS == LK.REASONS
    with pytest.raises(ValueError):
        pkg.LOBPCGSolver(pkg.DeviceMatrix(None), 43)
    with pytest.raises(ValueError):
        pkg.LOBPCGSolver(pkg.DeviceMatrix(None), 0)


def test_what_is_no_handle_is_refused_before_the_device(pkg):
    L = pkg._ffi.lib()
    junk = C.create_string_buffer(256)
    out = C.c_void_p(7)
    assert L.spl_lobpcg_create(junk, 4, C.byref(out)) == HANDLE and out.value == 7
    assert L.spl_lobpcg_create(None, 4, C.byref(out)) == HANDLE
    assert L.spl_lobpcg_set_preconditioner(junk, None, None, None) == HANDLE
    assert L.spl_lobpcg_set_preconditioner_amg(junk, None) == HANDLE
    info = (C.c_int64 * 8)()
    assert L.spl_lobpcg_info(junk, info) == HANDLE
    values = (C.c_double * 4)()
    assert L.spl_lobpcg_solve_dev(junk, 1, 1, 1e-8, 0.0, 10, None, 0, values, None, 0, values, info, None, None) == HANDLE
    assert L.spl_lobpcg_solve(junk, 1, 1, 1e-8, 0.0, 10, None, 0, None, None, 0, None, None, None) == HANDLE
    L.spl_lobpcg_free(None)
    empty = C.c_void_p()
    L.spl_lobpcg_free(C.byref(empty))
