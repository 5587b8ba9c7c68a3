"""Condition number estimates from the LU factors (spl_umfpack_di_condest, spl_umfpack_zi_condest): closed forms, dense
references, every factorisation path with its witness, the estimator at scale, statuses, determinism."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _matrix(pkg, S):
    S = S.tocsc()
    S.sort_indices()
    return pkg.Matrix(S.shape[1], S.shape[0], S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data)


def _factor(pkg, S):
    A = _matrix(pkg, S)
    return A, pkg.umfpack.factor(A, pkg.umfpack.analyze(A))


def _within(est, exact):
    """an estimate is a lower bound (up to numpy's own error, about kappa eps) and within a factor of 3"""
    kappa = exact
    assert est <= exact * (1.0 + max(1e-10, kappa * 1e-14)), (est, exact)
    assert est >= exact / 3.0, (est, exact)


def _check_witness(U, fact, A, r, norm):
    """solve A y = x with the library: ||y|| / ||x|| reaches the estimate of ||A^-1||"""
    x = r["witness"]
    y = U.linearSolve_(fact, U.UmfpackNormal, A, x)
    ratio = np.linalg.norm(y, norm) / np.linalg.norm(x, norm)
    if norm == 1:
        assert abs(ratio - r["norm_inv"]) <= 1e-8 * r["norm_inv"], (ratio, r["norm_inv"])
    else:
        assert ratio >= r["norm_inv"] * (1.0 - 1e-8), (ratio, r["norm_inv"])


def _check_dense(U, fact, A, D, witness=True):
    for norm in (1, np.inf):
        r = U.conditionEstimate(fact, A, norm=norm)
        assert abs(r["norm_A"] - np.linalg.norm(D, norm)) <= 1e-13 * r["norm_A"]
        _within(r["cond"], np.linalg.cond(D, norm))
        assert r["cond"] == r["norm_A"] * r["norm_inv"]
        assert 1 <= r["iterations"] <= 6 and 1 <= r["solves"] <= 11 and r["t"] == 2
        if witness:
            _check_witness(U, fact, A, r, norm)


def test_closed_forms(gpu, pkg):
    import scipy.sparse as sp
    U = pkg.umfpack
    rng = np.random.default_rng(1)
    d = rng.uniform(0.5, 2.0, 300) * np.where(rng.uniform(size=300) < 0.5, -1.0, 1.0)
    d[17], d[211] = 1e-3, -40.0
    A, f = _factor(pkg, sp.diags(d, format="csc"))
    for norm in (1, np.inf):
        r = U.conditionEstimate(f, A, norm=norm)
        assert r["norm_A"] == 40.0
        assert abs(r["cond"] - 40.0 / 1e-3) <= 1e-14 * 4e4, r
    # tridiag(-1, 2, -1), n odd: ||A^-1||_1 = (n + 1)^2 / 8, exact at the second iteration (A^-1 >= 0)
    n = 999
    T = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], (-1, 0, 1), format="csc")
    A, f = _factor(pkg, T)
    for norm in (1, np.inf):
        r = U.conditionEstimate(f, A, norm=norm)
        assert r["norm_A"] == 4.0
        assert abs(r["cond"] - (n + 1) ** 2 / 2.0) <= 1e-12 * (n + 1) ** 2 / 2.0, r
        assert r["iterations"] <= 3
    assert abs(U.condest(_matrix(pkg, T)) - (n + 1) ** 2 / 2.0) <= 1e-12 * (n + 1) ** 2 / 2.0


def _graded(rng, n):
    """kappa about 1e10: a well-conditioned random matrix scaled by rows and columns over five orders each"""
    R = rng.standard_normal((n, n)) + n ** 0.5 * 3.0 * np.eye(n)
    return np.diag(np.logspace(0, -5, n)) @ R @ np.diag(np.logspace(0, -5, n)[::-1] * rng.uniform(0.5, 1, n))


@pytest.mark.parametrize("kind", ["random", "graded", "hermitian", "complex_symmetric", "complex_general"])
def test_dense_references(gpu, pkg, kind):
    import scipy.sparse as sp
    U = pkg.umfpack
    rng = np.random.default_rng(sum(map(ord, kind)))
    n = 300 if kind == "random" else 200
    if kind == "random":
        D = rng.standard_normal((n, n)) * (rng.uniform(size=(n, n)) < 0.1) + np.diag(rng.uniform(1, 3, n))
    elif kind == "graded":
        D = _graded(rng, n)
    else:
        G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        G *= rng.uniform(size=(n, n)) < 0.1
        if kind == "hermitian":
            D = G + G.conj().T + np.diag(rng.uniform(-4, 4, n))
        elif kind == "complex_symmetric":
            D = G + G.T + np.diag(rng.uniform(2, 4, n) + 1j * rng.uniform(-1, 1, n))
        else:
            D = G + np.diag(rng.uniform(2, 4, n) * np.exp(2j * np.pi * rng.uniform(size=n)))
    if kind == "graded":
        assert np.linalg.cond(D, 1) > 1e9
    A, f = _factor(pkg, sp.csc_matrix(D))
    # the witness check compares one solve with the estimator's batched one: only where kappa keeps them together
    _check_dense(U, f, A, D, witness=np.linalg.cond(D, 1) <= 1e6)


def _tiny_blocks(rng, n, far):
    import scipy.sparse as sp
    off = np.zeros(n - 1)
    off[0::2] = 3.0
    return sp.diags([off, np.full(n, 1e-14), off, rng.uniform(-0.1, 0.1, n - far)], (-1, 0, 1, far), format="csc")


def _dominant_unsymmetric(rng, m):
    import scipy.sparse as sp
    T = sp.diags([rng.uniform(-1, 1, m - 1), rng.uniform(-1, 1, m - 1)], (-1, 1))
    I = sp.identity(m)
    d = rng.uniform(4.5, 6.0, m * m) * np.where(rng.uniform(size=m * m) < 0.3, -1.0, 1.0)
    return (sp.kron(I, T) + sp.kron(T, I) + sp.diags(d)).tocsc()


def _spd_not_dominant(rng, m):
    import scipy.sparse as sp
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], (-1, 0, 1))
    I = sp.identity(m)
    L = sp.kron(I, T) + sp.kron(T, I)
    B = sp.diags([rng.uniform(0.5, 1.0, m * m - 1)], [1])
    return (L @ L + 0.1 * (B + B.T) + 0.5 * sp.identity(m * m)).tocsc()


def _complex_convection(rng, m):
    """a complex unsymmetric 2-D operator, not diagonally dominant"""
    import scipy.sparse as sp
    T = sp.diags([np.full(m - 1, -1.0 + 0.3j), np.full(m, 2.5 + 0.0j), np.full(m - 1, -1.0 - 0.2j)], (-1, 0, 1))
    I = sp.identity(m)
    return (sp.kron(I, T) + sp.kron(T, I) - (1.0 + 0.5j) * sp.identity(m * m)
            + sp.diags(rng.uniform(-0.1, 0.1, m * m))).tocsc()


@pytest.mark.parametrize("case", ["band_pivot", "band_dominant", "band_speculation", "band_speculation_fails",
                                  "mf_dominant", "mf_speculation_ldlt", "mf_block_pivoting", "mf_static_pivot",
                                  "zi_native", "zi_embedding", "zi_embedding_band"])
def test_every_path(gpu, pkg, monkeypatch, case):
    import scipy.sparse as sp
    U = pkg.umfpack
    rng = np.random.default_rng(sum(map(ord, case)))
    monkeypatch.setenv("SPL_LU_METHOD", "band" if case.startswith("band") or case.endswith("band") else "mf")
    if case == "band_pivot":
        monkeypatch.setenv("SPL_LU_FORCE_PIVOT", "1")
        S, want = (sp.random(500, 500, density=0.01, random_state=rng) + sp.diags(rng.uniform(1, 2, 500))).tocsc(), 0
    elif case == "band_dominant":
        S, want = _dominant_unsymmetric(rng, 20), 1
    elif case == "band_speculation":
        S, want = _spd_not_dominant(rng, 20), 2
    elif case == "band_speculation_fails":
        monkeypatch.setenv("SPL_LU_STATIC_PIVOT", "0")
        S, want = _tiny_blocks(rng, 400, 5), None
    elif case == "mf_dominant":
        S, want = _dominant_unsymmetric(rng, 40), 3
    elif case == "mf_speculation_ldlt":
        S, want = _spd_not_dominant(rng, 36), 4
    elif case == "mf_block_pivoting":
        S, want = _tiny_blocks(rng, 900, 30), None
    elif case == "mf_static_pivot":
        monkeypatch.setenv("SPL_LU_BLOCK_PIVOT", "0")
        S, want = _tiny_blocks(rng, 900, 30), None
    else:
        monkeypatch.setenv("SPL_ZI_NATIVE", "1" if case == "zi_native" else "0")
        S, want = _complex_convection(rng, 24), None
    A, f = _factor(pkg, S)
    if want is not None:
        assert f.path == want
    D = S.toarray()
    assert np.linalg.cond(D, 1) <= 1e6
    _check_dense(U, f, A, D)
    if case == "zi_native":
        assert f.stats["complex_fronts"] == 1
    if case in ("band_speculation_fails", "mf_static_pivot"):
        assert f.path in (0, 5)  # the estimator's own solves replaced the failed speculation; the estimate is of A


def _laplacian3d(m):
    import scipy.sparse as sp
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], (-1, 0, 1))
    I = sp.identity(m)
    return (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsc()


def test_at_scale(gpu, pkg):
    import scipy.sparse as sp
    U = pkg.umfpack
    # 3-D Poisson 100^3: A^-1 >= 0 and A = A^T, so ||A^-1||_1 = max(A^-1 1), which one solve gives
    S = _laplacian3d(100)
    A, f = _factor(pkg, S)
    r = U.conditionEstimate(f, A)
    assert r["norm_A"] == 12.0
    exact = np.max(U.linearSolve_(f, U.UmfpackNormal, A, np.ones(S.shape[0])))
    assert abs(r["norm_inv"] - exact) <= 1e-10 * exact, (r, exact)
    # z I - A at 80^3, complex: the witness proves the estimate in both norms
    S = (3.0 + 0.5j) * sp.identity(80 ** 3, format="csc") - _laplacian3d(80).astype(np.complex128)
    A, f = _factor(pkg, S)
    for norm in (1, np.inf):
        r = U.conditionEstimate(f, A, norm=norm)
        assert abs(r["norm_A"] - (abs(3.0 + 0.5j - 6.0) + 6.0)) <= 1e-13 * r["norm_A"]
        _check_witness(U, f, A, r, norm)
        assert r["solves"] <= 11


def _raw(pkg, fact, sys=0, t=2, out=True, arrays=True, complex_call=False, mat=None):
    U = pkg.umfpack
    L = U._declare()
    nr, nc, ap, ai, ax = mat._tuple32()
    o = (C.c_double * 6)() if out else None
    pi, px = (pkg._ffi.p_i32, pkg._ffi.p_f64)
    args = (pi(ap), pi(ai), px(ax)) if arrays else (None, None, None)
    h = fact.value if hasattr(fact, "value") else fact
    if complex_call:
        st = L.spl_umfpack_zi_condest(sys, t, args[0], args[1], args[2], None, h, o, None, None)
    else:
        st = L.spl_umfpack_di_condest(sys, t, args[0], args[1], args[2], h, o, None)
    return st, (list(o) if out else None)


def test_statuses(gpu, pkg, monkeypatch):
    import scipy.sparse as sp
    U = pkg.umfpack
    S = sp.csc_matrix(np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]]))
    A, f = _factor(pkg, S)
    st, out = _raw(pkg, f, mat=A)
    assert st == 0 and abs(out[0] - np.linalg.cond(S.toarray(), 1)) <= 1e-13 * out[0] and out[5] == 2
    assert _raw(pkg, f, sys=2, mat=A)[0] == -13
    assert _raw(pkg, f, t=0, mat=A)[0] == -5
    assert _raw(pkg, f, t=17, mat=A)[0] == -5
    assert _raw(pkg, f, out=False, mat=A)[0] == -5
    assert _raw(pkg, f, arrays=False, mat=A)[0] == -5
    assert _raw(pkg, f, t=16, mat=A)[1][5] == 3  # t is at most n: X = I, the exact norm
    junk = (C.c_double * 64)()
    assert _raw(pkg, C.c_void_p(C.addressof(junk)), mat=A)[0] == -3
    assert _raw(pkg, None, mat=A)[0] == -3
    # the wrong value kind either way
    Z = sp.csc_matrix(S.toarray() * (1 + 1j))
    Az, fz = _factor(pkg, Z)
    assert _raw(pkg, fz, mat=A)[0] == -3
    assert _raw(pkg, f, complex_call=True, mat=Az)[0] == -3
    st, out = _raw(pkg, fz, complex_call=True, mat=Az)
    assert st == 0 and abs(out[0] - np.linalg.cond(Z.toarray(), 1)) <= 1e-13 * out[0]
    with pytest.raises(U.UmfpackError, match="complex"):
        U.conditionEstimate(f, Az)
    with pytest.raises(U.UmfpackError):
        U.conditionEstimate(f, A, norm=2)
    # rectangular object
    R = sp.csc_matrix(np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 7.0]]))
    Ar, fr = _factor(pkg, R)
    assert _raw(pkg, fr, mat=Ar)[0] == -13
    # singular factors: +inf, no solves
    monkeypatch.setenv("SPL_LU_FORCE_PIVOT", "1")
    monkeypatch.setenv("SPL_LU_METHOD", "band")
    Sg = sp.csc_matrix(np.array([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 1.0]]))
    Ag, fg = _factor(pkg, Sg)
    st, out = _raw(pkg, fg, mat=Ag)
    assert st == 1 and out[0] == np.inf and out[2] == np.inf and out[4] == 0
    # n = 1
    monkeypatch.delenv("SPL_LU_FORCE_PIVOT")
    A1, f1 = _factor(pkg, sp.csc_matrix(np.array([[-2.5]])))
    for norm in (1, np.inf):
        r = U.conditionEstimate(f1, A1, norm=norm)
        assert r["norm_A"] == 2.5 and abs(r["norm_inv"] - 0.4) <= 1e-15 and abs(r["cond"] - 1.0) <= 1e-15
        assert r["t"] == 1 and r["iterations"] == 1 and r["solves"] == 1
        assert np.abs(r["witness"]).tolist() == [1.0]


def test_deterministic_and_no_interference(gpu, pkg, monkeypatch):
    U = pkg.umfpack
    monkeypatch.setenv("SPL_LU_METHOD", "mf")
    rng = np.random.default_rng(5)
    S = _dominant_unsymmetric(rng, 40)  # unsymmetric multifrontal: the transposed solves have a chain set of their own
    A, f = _factor(pkg, S)
    b = rng.uniform(-1, 1, S.shape[0])
    U.linearSolve_(f, U.UmfpackTrans, A, b)
    x_before = U.linearSolve_(f, U.UmfpackNormal, A, b)
    report = f.solve_report
    for norm in (1, np.inf):
        r1 = U.conditionEstimate(f, A, norm=norm)
        r2 = U.conditionEstimate(f, A, norm=norm, t=2)
        assert r1["cond"] == r2["cond"] and np.array_equal(r1["witness"], r2["witness"])
        r4 = U.conditionEstimate(f, A, norm=norm, t=4)
        assert r4["t"] == 4 and r4["cond"] == U.conditionEstimate(f, A, norm=norm, t=4)["cond"]
    assert f.solve_report == report
    assert np.array_equal(U.linearSolve_(f, U.UmfpackNormal, A, b), x_before)
    # complex factors: the same
    Z = _complex_convection(rng, 20)
    Az, fz = _factor(pkg, Z)
    bz = rng.uniform(-1, 1, Z.shape[0]) + 1j * rng.uniform(-1, 1, Z.shape[0])
    U.linearSolve_(fz, U.UmfpackTrans, Az, bz)
    xz = U.linearSolve_(fz, U.UmfpackNormal, Az, bz)
    report = fz.solve_report
    r1, r2 = U.conditionEstimate(fz, Az), U.conditionEstimate(fz, Az)
    assert r1["cond"] == r2["cond"] and np.array_equal(r1["witness"], r2["witness"])
    assert fz.solve_report == report
    assert np.array_equal(U.linearSolve_(fz, U.UmfpackNormal, Az, bz), xz)
