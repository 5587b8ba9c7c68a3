"""Determinant, log-determinant and inertia read from the LU factors (umfpack_di_get_determinant,
spl_umfpack_di_log_determinant, spl_umfpack_inertia) on every factorisation path, against SciPy's SuperLU and closed
forms."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _perm_parity(p):
    p = np.asarray(p)
    seen = np.zeros(len(p), dtype=bool)
    odd = 0
    for i in range(len(p)):
        if seen[i]:
            continue
        length = 0
        j = i
        while not seen[j]:
            seen[j] = True
            j = p[j]
            length += 1
        odd ^= (length - 1) & 1
    return odd


def _ref_slogdet(S):
    """sign and ln|det| from SuperLU: Pr S Pc = L U with unit L"""
    import scipy.sparse.linalg as spla
    lu = spla.splu(S.tocsc())
    d = lu.U.diagonal()
    neg = int(np.sum(d < 0))
    sign = -1 if (neg + _perm_parity(lu.perm_r) + _perm_parity(lu.perm_c)) & 1 else 1
    return sign, float(np.sum(np.log(np.abs(d))))


def _matrix(pkg, S):
    S = S.tocsc()
    S.sort_indices()
    return pkg.Matrix(S.shape[1], S.shape[0], S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data)


def _check_against_scipy(U, fact, S):
    sign, logabs = U.logDeterminant(fact)
    rsign, rlog = _ref_slogdet(S)
    assert sign == rsign
    assert abs(logabs - rlog) <= 1e-10 * max(1.0, abs(rlog)), (logabs, rlog)
    mx, ex = U.determinant(fact)
    assert 1.0 <= abs(mx) < 10.0 and np.sign(mx) == sign
    assert abs((np.log(abs(mx)) + ex * np.log(10.0)) - rlog) <= 1e-10 * max(1.0, abs(rlog))


def _tiny_blocks(rng, n, far):
    """2 x 2 diagonal blocks [[1e-14, 3], [3, 1e-14]] with weak coupling: useless pivots in the given order"""
    import scipy.sparse as sp
    off = np.zeros(n - 1)
    off[0::2] = 3.0
    return sp.diags([off, np.full(n, 1e-14), off, rng.uniform(-0.1, 0.1, n - far)], (-1, 0, 1, far), format="csc")


def _dominant_unsymmetric(rng, m):
    import scipy.sparse as sp
    T = sp.diags([rng.uniform(-1, 1, m - 1), rng.uniform(-1, 1, m - 1)], (-1, 1))
    I = sp.identity(m)
    A = (sp.kron(I, T) + sp.kron(T, I)).tocsc()
    # column sums of |off-diagonal| <= 4: dominant; signs of the diagonal mixed, so det has a sign to get right
    d = rng.uniform(4.5, 6.0, m * m) * np.where(rng.uniform(size=m * m) < 0.3, -1.0, 1.0)
    return (A + sp.diags(d)).tocsc()


def _spd_not_dominant(rng, m):
    """symmetric positive definite, not diagonally dominant (a speculation that holds)"""
    import scipy.sparse as sp
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], (-1, 0, 1))
    I = sp.identity(m)
    L = sp.kron(I, T) + sp.kron(T, I)
    B = sp.diags([rng.uniform(0.5, 1.0, m * m - 1)], [1])
    return (L @ L + 0.1 * (B + B.T) + 0.5 * sp.identity(m * m)).tocsc()


@pytest.mark.parametrize("case", ["band_pivot", "band_dominant", "band_speculation", "band_speculation_fails",
                                  "band_speculation_fails_odd", "mf_dominant", "mf_speculation_ldlt",
                                  "mf_block_pivoting", "mf_block_pivoting_odd", "mf_static_pivot",
                                  "mf_static_pivot_odd"])
def test_every_path_matches_superlu(gpu, pkg, monkeypatch, case):
    import scipy.sparse as sp
    U = pkg.umfpack
    rng = np.random.default_rng(sum(map(ord, case)))
    # _tiny_blocks: every [[1e-14, 3], [3, 1e-14]] pair costs one interchange (ipiv, the threshold pivoting inside the
    # blocks, or the transversal of static pivoting) and then gives two pivots of about +3: the sign of det, (-1)^pairs,
    # comes from the interchanges alone.  "_odd": an odd number of pairs, so the sign is -1 and only the parity of the
    # interchanges gets it right
    odd = case.endswith("_odd")
    pairs_band, pairs_mf = (199, 449) if odd else (200, 450)
    case = case[:-4] if odd else case
    if case == "band_pivot":
        monkeypatch.setenv("SPL_LU_FORCE_PIVOT", "1")
        monkeypatch.setenv("SPL_LU_METHOD", "band")
        S = (sp.random(500, 500, density=0.01, random_state=rng) + sp.diags(rng.uniform(-1, 1, 500))).tocsc()
        want, block = 0, None
    elif case == "band_dominant":
        monkeypatch.setenv("SPL_LU_METHOD", "band")
        S, want, block = _dominant_unsymmetric(rng, 20), 1, None
    elif case == "band_speculation":
        monkeypatch.setenv("SPL_LU_METHOD", "band")
        S, want, block = _spd_not_dominant(rng, 20), 2, None
    elif case == "band_speculation_fails":
        monkeypatch.setenv("SPL_LU_METHOD", "band")
        monkeypatch.setenv("SPL_LU_STATIC_PIVOT", "0")
        S, want, block = _tiny_blocks(rng, 2 * pairs_band, 5), 0, None
    elif case == "mf_dominant":
        monkeypatch.setenv("SPL_LU_METHOD", "mf")
        S, want, block = _dominant_unsymmetric(rng, 40), 3, 0
    elif case == "mf_speculation_ldlt":
        monkeypatch.setenv("SPL_LU_METHOD", "mf")
        S, want, block = _spd_not_dominant(rng, 36), 4, 0
    elif case == "mf_block_pivoting":
        monkeypatch.setenv("SPL_LU_METHOD", "mf")
        S, want, block = _tiny_blocks(rng, 2 * pairs_mf, 30), 4, 1
    else:
        monkeypatch.setenv("SPL_LU_METHOD", "mf")
        monkeypatch.setenv("SPL_LU_BLOCK_PIVOT", "0")
        S, want, block = _tiny_blocks(rng, 2 * pairs_mf, 30), 5, 0
    A = _matrix(pkg, S)
    fact = U.factor(A, U.analyze(A))
    before = fact.path
    _check_against_scipy(U, fact, S)
    assert fact.path == want, (before, fact.path)
    if case in ("band_speculation_fails", "mf_block_pivoting", "mf_static_pivot"):
        assert _ref_slogdet(S)[0] == (-1 if odd else 1)  # the case does test the parity of the interchanges
        assert U.logDeterminant(fact)[0] == (-1 if odd else 1)
    if case == "band_speculation_fails":
        assert before == 2  # the failed speculation was replaced by partial pivoting before the pivots were read
    if case == "mf_static_pivot":
        assert before == 4
    if block is not None:
        assert fact.stats["block_pivoting"] == block
    # the second call reads the same factors: bit-identical
    assert U.logDeterminant(fact) == U.logDeterminant(fact)
    assert U.determinant(fact) == U.determinant(fact)


def _laplacian3d(m):
    import scipy.sparse as sp
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], (-1, 0, 1))
    I = sp.identity(m)
    return (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsc()


def test_laplacian_closed_forms(gpu, pkg):
    import scipy.sparse as sp
    U = pkg.umfpack
    # 1-D: det = n + 1
    n = 999
    T = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], (-1, 0, 1), format="csc")
    mx, ex = U.det(_matrix(pkg, T))
    assert 1.0 <= mx < 10.0 and ex in (2, 3) and abs(mx * 10.0 ** ex - (n + 1)) <= 1e-12 * (n + 1)
    # 3-D at 100^3: ln det = sum ln(l_i + l_j + l_k), l_i = 2 - 2 cos(i pi / (m + 1)); L D L^T on the tree
    m = 100
    S = _laplacian3d(m)
    lam = 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
    ref = float(np.sum(np.log(lam[:, None, None] + lam[None, :, None] + lam[None, None, :])))
    A = _matrix(pkg, S)
    an = U.analyze(A)
    fact = U.factor(A, an)
    assert fact.path == 3
    sign, logabs = U.logDeterminant(fact)
    assert sign == 1 and abs(logabs - ref) <= 1e-11 * abs(ref), (logabs, ref)
    assert U.inertia(fact) == (m ** 3, 0, 0)
    del fact
    neg = _matrix(pkg, -S)
    fneg = U.factor(neg, U.analyze(neg))
    sign, logabs = U.logDeterminant(fneg)
    assert sign == 1 and abs(logabs - ref) <= 1e-11 * abs(ref)  # (-1)^n, n even
    assert U.inertia(fneg) == (0, m ** 3, 0)


@pytest.mark.parametrize("method", ["band", "mf"])
@pytest.mark.parametrize("fraction", [0.03, 0.4, 0.8])
def test_inertia_of_shifted_laplacian(gpu, pkg, monkeypatch, method, fraction):
    import scipy.sparse as sp
    U = pkg.umfpack
    monkeypatch.setenv("SPL_LU_METHOD", method)
    m = 40
    lam = 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
    ev = np.sort((lam[:, None] + lam[None, :]).ravel())
    # sigma in the widest gap of the spectrum near the wanted fraction of it below
    k0 = int(fraction * m * m)
    k = max(range(k0 - 20, k0 + 20), key=lambda i: ev[i + 1] - ev[i])
    sigma = 0.5 * (ev[k] + ev[k + 1])
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], (-1, 0, 1))
    I = sp.identity(m)
    S = (sp.kron(I, T) + sp.kron(T, I) - sigma * sp.identity(m * m)).tocsc()
    mu = ev - sigma
    assert np.min(np.abs(mu)) > 1e-4  # sigma is away from the spectrum
    A = _matrix(pkg, S)
    fact = U.factor(A, U.analyze(A))
    sign, logabs = U.logDeterminant(fact)
    below = int(np.sum(mu < 0))
    assert sign == (-1) ** below
    ref = float(np.sum(np.log(np.abs(mu))))
    # (factors without interchanges of an INDEFINITE matrix: the refined solves are backward stable, the pivots carry the
    # growth — 1e-10 relative on log|det| measured at the widest; the sign and the counts are exact)
    assert abs(logabs - ref) <= 1e-8 * max(1.0, abs(ref))
    st = fact.stats
    congruence = st["path"] in (1, 2, 3, 4) and st["block_pivoting"] == 0
    if congruence:
        assert U.inertia(fact) == (m * m - below, below, 0)
    else:
        with pytest.raises(U.UmfpackError, match="path %d" % st["path"]):
            U.inertia(fact)


def test_inertia_refuses_what_is_not_a_congruence(gpu, pkg, monkeypatch):
    U = pkg.umfpack
    rng = np.random.default_rng(5)
    monkeypatch.setenv("SPL_LU_METHOD", "mf")
    S = _dominant_unsymmetric(rng, 40)  # no interchanges, but A != A^T
    A = _matrix(pkg, S)
    fact = U.factor(A, U.analyze(A))
    assert fact.path == 3
    with pytest.raises(U.UmfpackError, match="path 3.*not symmetric"):
        U.inertia(fact)
    S = _tiny_blocks(rng, 900, 30)  # block pivoting
    A = _matrix(pkg, S)
    fact = U.factor(A, U.analyze(A))
    with pytest.raises(U.UmfpackError, match="threshold pivoting"):
        U.inertia(fact)
    assert fact.stats["block_pivoting"] == 1
    monkeypatch.setenv("SPL_LU_FORCE_PIVOT", "1")
    fact = U.factor(A, U.analyze(A))
    with pytest.raises(U.UmfpackError, match="path 0"):
        U.inertia(fact)


def _raw(pkg, fact, with_ex=True, with_mx=True):
    L = pkg.umfpack._declare()
    mx, ex = C.c_double(7.0), C.c_double(7.0)
    info = (C.c_double * 90)()
    st = L.umfpack_di_get_determinant(C.byref(mx) if with_mx else None, C.byref(ex) if with_ex else None,
                                      fact.value, info)
    assert info[0] == st
    return st, mx.value, ex.value


def test_edge_statuses(gpu, pkg):
    import scipy.sparse as sp
    U = pkg.umfpack
    n = 4
    big = _matrix(pkg, sp.diags(np.full(n, 1e300), format="csc"))
    fb = U.factor(big, U.analyze(big))
    st, mx, _ = _raw(pkg, fb, with_ex=False)
    assert st == 3 and mx == np.inf
    st, mx, ex = _raw(pkg, fb)
    assert st == 0 and 1.0 <= mx < 10.0 and abs(np.log10(mx) + ex - 1200.0) < 1e-12
    small = _matrix(pkg, sp.diags(np.full(n, -1e-300), format="csc"))
    fs = U.factor(small, U.analyze(small))
    st, mx, _ = _raw(pkg, fs, with_ex=False)
    assert st == 2 and mx == 0.0
    st, mx, ex = _raw(pkg, fs)
    assert st == 0 and 1.0 <= mx < 10.0 and abs(np.log10(mx) + ex + 1200.0) < 1e-12  # (-1)^4 > 0
    assert U.logDeterminant(fs)[0] == 1
    # a zero pivot: singular
    Z = sp.csc_matrix(np.array([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 1.0]]))
    fz = U.factor(_matrix(pkg, Z), U.analyze(_matrix(pkg, Z)))
    st, mx, ex = _raw(pkg, fz)
    assert st == 1 and mx == 0.0 and ex == 0.0
    assert U.logDeterminant(fz) == (0, -np.inf)
    # rectangular: 3 x 2
    R = sp.csc_matrix(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]))
    fr = U.factor(_matrix(pkg, R), U.analyze(_matrix(pkg, R)))
    assert _raw(pkg, fr)[0] == -13
    # no Mx
    assert _raw(pkg, fb, with_mx=False)[0] == -5
    # complex factors
    Zc = sp.csc_matrix(np.array([[2.0 + 1.0j, 0.5], [0.25j, 3.0]]))
    Ac = pkg.Matrix(2, 2, Zc.indptr.astype(np.int64), Zc.indices.astype(np.int64), Zc.data)
    fc = U.factor(Ac, U.analyze(Ac))
    with pytest.raises(U.UmfpackError, match="complex"):
        U.determinant(fc)
    with pytest.raises(U.UmfpackError, match="complex"):
        U.logDeterminant(fc)
    with pytest.raises(U.UmfpackError, match="complex"):
        U.inertia(fc)
    # the C entry point on a complex object: invalid Numeric object
    assert _raw(pkg, fc)[0] == -3


def test_solve_after_determinant_is_unchanged(gpu, pkg, monkeypatch):
    """the check a determinant call makes on speculative factors leaves later solves as they would have been"""
    U = pkg.umfpack
    monkeypatch.setenv("SPL_LU_METHOD", "mf")
    rng = np.random.default_rng(11)
    for S in (_tiny_blocks(rng, 900, 30), _spd_not_dominant(rng, 36)):
        A = _matrix(pkg, S)
        b = S @ rng.uniform(0.5, 1.5, S.shape[0])
        f1 = U.factor(A, U.analyze(A))
        U.determinant(f1)
        x1 = U.linearSolve_(f1, U.UmfpackNormal, A, b)
        f2 = U.factor(A, U.analyze(A))
        x2 = U.linearSolve_(f2, U.UmfpackNormal, A, b)
        assert f1.path == f2.path
        assert np.array_equal(x1, x2)
    # the check of a first determinant call on speculative factors is not reported as the caller's last solve
    S = _tiny_blocks(rng, 900, 30)
    A = _matrix(pkg, S)
    f = U.factor(A, U.analyze(A))
    assert f.path == 4
    U.linearSolve_(f, U.UmfpackNormal, A, S @ np.ones(900))
    report = f.solve_report
    U.logDeterminant(f)
    assert f.solve_report == report
