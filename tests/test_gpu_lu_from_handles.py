"""LU from device-resident matrix handles: spl_umfpack_{di,zi}_{symbolic,numeric}_dev (include/umfpack_hip.h),
`analyzeDevice` / `factorDevice` of the Python mirror.

The comparison partner is always the HOST-BORN object of the same matrix (`analyze` / `factor` on the CSC arrays):
both routes put the same two images on the device and the factorisation is deterministic, so paths, figures,
determinants and solutions are required to be equal bit for bit.  Independently of that, the solutions of the
handle-born object are checked against a residual computed on the host with scipy."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bwd(S, x, b):
    """componentwise backward error max_i |r_i| / (|A| |x| + |b|)_i (what the solves drive below 1e-13)"""
    r = np.abs(S @ x - b)
    den = abs(S) @ np.abs(x) + np.abs(b)
    return float(np.max(r / np.where(den > 0, den, 1.0)))


def _mat(pkg, S):
    S = S.tocsc()
    S.sort_indices()
    return pkg.Matrix(S.shape[1], S.shape[0], S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data)


def _handle(pkg, M):
    return pkg.DeviceMatrix.from_csc_complex(M) if M.is_complex else pkg.DeviceMatrix.from_csc(M)


def _grid(m, dim, diag=2.0):
    import scipy.sparse as sp
    T = sp.diags([-np.ones(m - 1), diag * np.ones(m), -np.ones(m - 1)], (-1, 0, 1))
    I = sp.identity(m)
    if dim == 2:
        return sp.csc_matrix(sp.kron(I, T) + sp.kron(T, I))
    return sp.csc_matrix(sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I))


# ---- the constructions of tests/test_gpu_umfpack.py, one per path ------------------------------------------------------
def _dominant_unsymmetric_grid(m):
    """5-point pattern, unsymmetric values, diagonal 4.5 above the column sums of the rest: column dominant"""
    rng = np.random.default_rng(41)
    S = _grid(m, 2)
    S.data = S.data * rng.uniform(0.5, 1.0, S.nnz)
    S.setdiag(4.5)
    return sp_csc(S)


def sp_csc(S):
    import scipy.sparse as sp
    S = sp.csc_matrix(S)
    S.sort_indices()
    return S


def _btb(n):
    """B^T B + 0.05 I of a banded B: positive definite, NOT diagonally dominant — a speculation that holds"""
    import scipy.sparse as sp
    rng = np.random.default_rng(23)
    Bm = sp.diags([rng.uniform(0.5, 1.5, n - abs(d)) for d in (-7, -1, 0, 1, 3)], (-7, -1, 0, 1, 3), format="csc")
    S = sp_csc(Bm.T @ Bm + 0.05 * sp.identity(n))
    assert np.any(np.abs(S.diagonal()) < np.asarray(abs(S).sum(axis=0)).ravel() - np.abs(S.diagonal()))
    return S


def _tiny_blocks(m):
    """2 x 2 diagonal blocks [[1e-14, 3], [3, 1e-14]] plus a weak coupling: useless pivots in the given order; the
    threshold pivoting inside the diagonal blocks of the fronts takes the 3s"""
    import scipy.sparse as sp
    rng = np.random.default_rng(41)
    n = m * m
    off = np.zeros(n - 1)
    off[0::2] = 3.0
    return sp_csc(sp.diags([off, np.full(n, 1e-14), off, rng.uniform(-0.1, 0.1, n - m)], (-1, 0, 1, m), format="csc"))


def _tiny_diagonal_mesh(m):
    """random unsymmetric values on a 5-point pattern with a diagonal of 1e-12: the factors without interchanges are
    useless, the first solve refactors with static pivoting (path 5)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(m)
    S = sp.csc_matrix(_grid(m, 2))
    S.data = rng.uniform(-1.0, 1.0, S.nnz)
    S.setdiag(1e-12 * rng.uniform(0.5, 1.0, S.shape[0]))
    return sp_csc(S)


# (name, environment, matrix, path of the fresh object (None: not pinned), path after the solves, backward error bound:
# the product's contract of 1e-13 — 1e-12 for the 1e-14 family, whose existing test uses 1e-12)
_REAL_CASES = [
    ("path0_forced_pivoting", {"SPL_LU_FORCE_PIVOT": "1"}, lambda: _dominant_unsymmetric_grid(30), 0, 0, 1e-13),
    ("path1_band_dominant", {"SPL_LU_METHOD": "band"}, lambda: _dominant_unsymmetric_grid(30), 1, 1, 1e-13),
    ("path2_band_speculation", {"SPL_LU_METHOD": "band"}, lambda: _btb(600), 2, 2, 1e-13),
    ("path3_tree_dominant", {"SPL_LU_METHOD": "mf"}, lambda: _dominant_unsymmetric_grid(45), 3, 3, 1e-13),
    ("path4_tree_block_pivoting", {"SPL_LU_METHOD": "mf"}, lambda: _tiny_blocks(40), 4, 4, 1e-12),
    ("path5_static_pivoting", {"SPL_LU_METHOD": "mf"}, lambda: _tiny_diagonal_mesh(300), None, 5, 1e-13),
]


def _device_rhs(torch, rng, k, n, cplx):
    B = rng.normal(size=(k, n)) + (1j * rng.normal(size=(k, n)) if cplx else 0.0)
    return torch.from_numpy(np.ascontiguousarray(B)).cuda()


def _compare_objects(torch, pkg, S, M, fh, fd, rng, bound):
    """handle-born fd against host-born fh: path, figures, solutions of the same device right-hand sides (A and A^T or
    A^H; 1 and 5 columns) bit for bit, path again; the handle-born solutions against scipy's residual"""
    import scipy.sparse as sp
    U = pkg.umfpack
    n = S.shape[0]
    cplx = bool(M.is_complex)
    assert fd.path == fh.path and fd.stats == fh.stats and fd.status == fh.status
    for mode, op in ((U.UmfpackNormal, S), (U.UmfpackTrans, sp.csc_matrix(S.conj().T))):
        for k in (1, 5):
            B = _device_rhs(torch, rng, k, n, cplx)
            Xh = U.linearSolveManyDevice_(fh, mode, M, B).cpu().numpy()
            Xd = U.linearSolveManyDevice_(fd, mode, None, B).cpu().numpy()
            assert np.array_equal(Xd.view(np.float64), Xh.view(np.float64)), (mode, k, float(np.max(np.abs(Xd - Xh))))
            Bh = B.cpu().numpy()
            for c in range(k):
                err = _bwd(op, Xd[c], Bh[c])
                print("backward error mode %d k %d column %d: %.3g" % (mode, k, c, err))
                assert err <= bound
    assert fd.path == fh.path and fd.stats == fh.stats  # a replaced speculation is replaced on both sides


@pytest.mark.parametrize("case", _REAL_CASES, ids=[c[0] for c in _REAL_CASES])
def test_real_every_path_has_the_bits_of_the_host_route(gpu, pkg, case, monkeypatch):
    name, env, build, path_fresh, path_after, bound = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    U = pkg.umfpack
    S = build()
    M = _mat(pkg, S)
    fh = U.factor(M, U.analyze(M))
    if path_fresh is not None:
        assert fh.path == path_fresh  # a matrix that misses its path fails here instead of testing less
    H = _handle(pkg, M)
    fd = U.factorDevice(H, U.analyzeDevice(H))
    assert fd.path == fh.path and fd.stats == fh.stats
    if path_fresh is not None:  # (on unchecked speculative factors a determinant call may replace them: after the solves)
        dh, dd = U.determinant(fh), U.determinant(fd)
        assert np.array([dh[0]]).tobytes() == np.array([dd[0]]).tobytes() and dh[1] == dd[1], (dh, dd)
    _compare_objects(gpu, pkg, S, M, fh, fd, np.random.default_rng(3), bound)
    assert fh.path == path_after and fd.path == path_after
    dh, dd = U.determinant(fh), U.determinant(fd)
    assert np.array([dh[0]]).tobytes() == np.array([dd[0]]).tobytes() and dh[1] == dd[1], (dh, dd)


# ---- complex: every embedding (the constructions of tests/test_gpu_complex.py) ------------------------------------------
def _complex_imaginary_diagonal(n):
    """unsymmetric, every diagonal entry purely imaginary: every complex row swaps its two real equations"""
    import scipy.sparse as sp
    rng = np.random.default_rng(21)
    k = 4 * n
    S = sp.csc_matrix((rng.normal(size=k) + 1j * rng.normal(size=k), (rng.integers(0, n, k), rng.integers(0, n, k))),
                      shape=(n, n))
    S = sp.csc_matrix(S - sp.diags(S.diagonal()) + sp.diags(np.where(np.arange(n) % 2 == 0, 30.0j, -26.0j)))
    return sp_csc(S)


def _complex_mixed_diagonal(n, empty_rows=()):
    """unsymmetric; the diagonal entries are imaginary-dominant in about half of the rows, chosen at random (so that the
    flags follow no period of the kernels' tiles or lanes): a flag read for the wrong row, or by column, changes the
    embedding.  empty_rows: rows without any entry (a singular matrix) inside the tiles of the embedding kernel."""
    import scipy.sparse as sp
    rng = np.random.default_rng(33)
    k = 4 * n
    S = sp.csc_matrix((rng.normal(size=k) + 1j * rng.normal(size=k), (rng.integers(0, n, k), rng.integers(0, n, k))),
                      shape=(n, n))
    imag = rng.random(n) < 0.5
    assert 0.3 * n < imag.sum() < 0.7 * n
    d = np.where(imag, rng.uniform(-2.0, 2.0, n) + 1j * rng.choice([-28.0, 30.0], n), rng.choice([-27.0, 29.0], n) + 1j * rng.uniform(-2.0, 2.0, n))
    S = sp.lil_matrix(S - sp.diags(S.diagonal()) + sp.diags(d))
    for r in empty_rows:
        S[r, :] = 0
    S = sp_csc(S)
    S.eliminate_zeros()
    return sp_csc(S)


def _complex_shift(m, z=0.7 - 0.4j):
    """z B - A on a 3-D grid, B a positive diagonal: complex symmetric, not Hermitian (a FEAST contour point)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(m)
    A = _grid(m, 3)
    return sp_csc(z * sp.diags(rng.uniform(0.8, 1.25, A.shape[0])) - A)


def _complex_unsymmetric_mesh(m):
    rng = np.random.default_rng(17)
    P = _grid(m, 2).astype(np.complex128)
    P.data = rng.uniform(-1, 1, P.nnz) + 1j * rng.uniform(-1, 1, P.nnz)
    w = np.asarray(abs(P).sum(axis=0)).ravel()
    P.setdiag(2.0 * w + 0j)
    return sp_csc(P)


_COMPLEX_CASES = [
    ("a_swapped_pairs_band", {"SPL_LU_METHOD": "band"}, lambda: _complex_imaginary_diagonal(400)),
    ("a2_mixed_swaps_band", {"SPL_LU_METHOD": "band"}, lambda: _complex_mixed_diagonal(700)),
    ("b_native_symmetric", {"SPL_LU_METHOD": "mf", "SPL_ZI_NATIVE": "1"}, lambda: _complex_shift(13)),
    ("c_congruence", {"SPL_LU_METHOD": "mf", "SPL_ZI_NATIVE": "0", "SPL_ZI_SYMMETRIC": "1"}, lambda: _complex_shift(13)),
    ("d_native_unsymmetric", {"SPL_LU_METHOD": "mf", "SPL_ZI_NATIVE": "1"}, lambda: _complex_unsymmetric_mesh(48)),
]


@pytest.mark.parametrize("case", _COMPLEX_CASES, ids=[c[0] for c in _COMPLEX_CASES])
def test_complex_every_embedding_has_the_bits_of_the_host_route(gpu, pkg, case, monkeypatch):
    """Bit equality is required of all: (a), (a2), (b), (d) only move and negate values — (a) swaps every pair, as the
    contract's case asks, (a2) about half of them, which makes the flags themselves observable; the units of (c), the congruence
    embedding, are computed by the same host function on both routes (from the n diagonal entries the handle route
    brings down) and multiplied in the same order with contraction off."""
    name, env, build = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    U = pkg.umfpack
    S = build()
    M = _mat(pkg, S)
    assert M.is_complex
    fh = U.factor(M, U.analyze(M))
    st = fh.stats
    if name[0] == "a":
        assert fh.path in (0, 1, 2) and st["fronts"] == 0
    elif name[0] == "b":
        assert fh.path in (3, 4) and st["complex_fronts"] == 1
    elif name[0] == "c":
        monkeypatch.setenv("SPL_ZI_SYMMETRIC", "0")
        general = U.factor(M, U.analyze(M)).stats
        monkeypatch.setenv("SPL_ZI_SYMMETRIC", "1")
        # the symmetric embedding runs the tree in its L D L^T mode: half the flops of the general one
        assert fh.path in (3, 4) and st["complex_fronts"] == 0 and st["flops"] == 0.5 * general["flops"]
    else:
        assert fh.path in (3, 4) and st["complex_fronts"] == 1
    H = _handle(pkg, M)
    assert H.is_complex
    fd = U.factorDevice(H, U.analyzeDevice(H))
    assert fd.complex
    _compare_objects(gpu, pkg, S, M, fh, fd, np.random.default_rng(5), 1e-13)


def test_empty_rows_inside_a_tile_of_the_embedding(gpu, pkg, monkeypatch):
    """rows without entries (the embedding kernel finds the row of an entry by bisection over a tile's row pointers,
    which has to step over them; the diagonal pass finds no diagonal there).  Such a matrix is singular, so there are
    no solutions to compare: the two routes must agree on the status (singular), the path, the figures and the exact
    norm the object computes from its device copy of A — a check of the layout, not of every value."""
    monkeypatch.setenv("SPL_LU_METHOD", "band")
    U = pkg.umfpack
    S = _complex_mixed_diagonal(700, empty_rows=(0, 3, 4, 255, 256, 257, 511, 699))
    assert np.count_nonzero(np.diff(S.tocsr().indptr) == 0) == 8
    M = _mat(pkg, S)
    H = _handle(pkg, M)
    fh = U.factor(M, U.analyze(M))
    fd = U.factorDevice(H, U.analyzeDevice(H))
    assert fh.status == 1 and fd.status == 1
    assert fd.path == fh.path and fd.stats == fh.stats
    for norm in (1, np.inf):
        eh, ed = U.conditionEstimate(fh, M, norm=norm), U.conditionEstimate(fd, M, norm=norm)
        assert ed["norm_A"] == eh["norm_A"] and ed["cond"] == eh["cond"]
    assert abs(eh["norm_A"] - abs(S).sum(axis=1).max()) <= 1e-12 * eh["norm_A"]  # norm = inf: the largest row sum of moduli


# ---- the device pipeline end to end (Feast.hs:210-218) -------------------------------------------------------------------
def test_contour_points_assembled_and_factored_on_the_device(gpu, pkg, monkeypatch):
    """real handles A, B -> to_complex -> ze B - A on the device for three ze -> ONE analyzeDevice, three factorDevice
    -> solves with NULL arrays; against host lin -> analyze -> factor -> solve.  No matrix moves to the host between
    the creation of the handles and the reading of the solutions."""
    import scipy.sparse as sp
    monkeypatch.setenv("SPL_LU_METHOD", "mf")
    U = pkg.umfpack
    rng = np.random.default_rng(9)
    A = _grid(12, 3)
    n = A.shape[0]
    B = sp_csc(sp.diags(rng.uniform(0.8, 1.25, n)))
    MA, MB = _mat(pkg, A), _mat(pkg, B)
    HA, HB = pkg.DeviceMatrix.from_csc(MA).to_complex(), pkg.DeviceMatrix.from_csc(MB).to_complex()
    Bd = _device_rhs(gpu, rng, 4, n, True)
    zes = (0.7 - 0.4j, 4.0 + 0.01j, -0.2 + 3.0j)
    an_dev = None
    X_dev = []
    for ze in zes:
        HC = HB.lin(ze, HA, -1.0)
        if an_dev is None:
            an_dev = U.analyzeDevice(HC)
        fd = U.factorDevice(HC, an_dev)
        HC.free()
        X_dev.append((fd.path, fd.stats, U.linearSolveManyDevice_(fd, U.UmfpackNormal, None, Bd)))
    an_host = None
    Bh = Bd.cpu().numpy()
    for ze, (path, stats, Xd) in zip(zes, X_dev):
        MC = pkg.lin(ze, MB, -1.0, MA)
        if an_host is None:
            an_host = U.analyze(MC)
        fh = U.factor(MC, an_host)
        Xh = U.linearSolveManyDevice_(fh, U.UmfpackNormal, MC, Bd).cpu().numpy()
        assert (fh.path, fh.stats) == (path, stats)
        assert np.array_equal(Xd.cpu().numpy().view(np.float64), Xh.view(np.float64)), ze
        Sc = sp_csc(ze * B - A)
        for c in range(4):
            assert _bwd(Sc, Xh[c], Bh[c]) <= 1e-13


# ---- pattern check ---------------------------------------------------------------------------------------------------------
def _same_counts_other_place(n=60):
    """two patterns with the same number of entries in every row and every column, one 2 x 2 minor placed the other
    way round: the diagonal plus (r1, c1), (r2, c2) against the diagonal plus (r1, c2), (r2, c1)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(2)
    base = (sp.identity(n) * 4.0).tolil()
    for i in range(n - 1):
        base[i, i + 1] = -1.0
        base[i + 1, i] = -1.0
    r1, r2, c1, c2 = 5, 20, 30, 44
    P, Q = base.copy(), base.copy()
    P[r1, c1] = P[r2, c2] = 0.5
    Q[r1, c2] = Q[r2, c1] = 0.5
    P, Q = sp_csc(P), sp_csc(Q)
    P.data = P.data * rng.uniform(0.9, 1.0, P.nnz)
    return P, Q


@pytest.mark.parametrize("cplx", [False, True])
def test_another_pattern_with_the_same_counts_is_refused(gpu, pkg, cplx):
    import scipy.sparse as sp
    U = pkg.umfpack
    P, Q = _same_counts_other_place()
    for ax in (0, 1):  # only an exact compare can tell them apart
        assert np.array_equal(np.diff(sp.csc_matrix(P).indptr) if ax == 0 else np.diff(sp.csr_matrix(P).indptr),
                              np.diff(sp.csc_matrix(Q).indptr) if ax == 0 else np.diff(sp.csr_matrix(Q).indptr))
    assert P.nnz == Q.nnz and (P != Q).nnz > 0
    if cplx:
        P, Q = sp_csc(P * (1.0 + 0.25j)), sp_csc(Q * (1.0 + 0.25j))
    MP, MQ = _mat(pkg, P), _mat(pkg, Q)
    HP, HQ = _handle(pkg, MP), _handle(pkg, MQ)
    for an in (U.analyze(MP), U.analyzeDevice(HP)):
        with pytest.raises(U.UmfpackError) as e:
            U.factorDevice(HQ, an)
        assert e.value.status == -11  # UMFPACK_ERROR_different_pattern
        U.factorDevice(HP, an)  # the analysed pattern passes, before and after a refusal
        with pytest.raises(U.UmfpackError) as e:
            U.factorDevice(HQ, an)
        assert e.value.status == -11
    with pytest.raises(U.UmfpackError) as e:
        U.factor(MQ, U.analyzeDevice(HP))
    assert e.value.status == -11


@pytest.mark.parametrize("cplx", [False, True])
def test_objects_of_either_origin_serve_calls_of_either_origin(gpu, pkg, cplx, monkeypatch):
    """host Symbolic + numeric_dev, and symbolic_dev + host numeric: the bits of the all-host route"""
    monkeypatch.setenv("SPL_LU_METHOD", "mf")
    U = pkg.umfpack
    S = _complex_unsymmetric_mesh(40) if cplx else _dominant_unsymmetric_grid(40)
    M = _mat(pkg, S)
    H = _handle(pkg, M)
    fh = U.factor(M, U.analyze(M))
    rng = np.random.default_rng(1)
    B = _device_rhs(gpu, rng, 3, S.shape[0], cplx)
    want = U.linearSolveManyDevice_(fh, U.UmfpackNormal, M, B).cpu().numpy()
    for f in (U.factorDevice(H, U.analyze(M)), U.factor(M, U.analyzeDevice(H))):
        assert f.path == fh.path and f.stats == fh.stats
        got = U.linearSolveManyDevice_(f, U.UmfpackNormal, H, B).cpu().numpy()
        assert np.array_equal(got.view(np.float64), want.view(np.float64))
        one = U.linearSolve_(f, U.UmfpackNormal, M, B[0].cpu().numpy())  # every existing entry point takes the object
        assert np.array_equal(one.view(np.float64), U.linearSolve_(fh, U.UmfpackNormal, M, B[0].cpu().numpy()).view(np.float64))
        est = U.conditionEstimate(f, M)
        assert est["cond"] == U.conditionEstimate(fh, M)["cond"]


# ---- borrowing -------------------------------------------------------------------------------------------------------------
def test_the_handle_is_borrowed(gpu, pkg, monkeypatch):
    """the handle is unchanged by the calls and may be freed before the first solve — also before a solve that makes a
    speculative object refactor from its own copy (the tiny-diagonal matrix: static pivoting, path 5)"""
    import scipy.sparse as sp
    monkeypatch.setenv("SPL_LU_METHOD", "mf")
    U = pkg.umfpack
    S = _tiny_diagonal_mesh(300)
    M = _mat(pkg, S)
    H = _handle(pkg, M)
    before = [a.copy() for a in H.export_csr()]
    fd = U.factorDevice(H, U.analyzeDevice(H))
    after = H.export_csr()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    H.free()
    fh = U.factor(M, U.analyze(M))
    rng = np.random.default_rng(4)
    for mode, op in ((U.UmfpackNormal, S), (U.UmfpackTrans, sp.csc_matrix(S.T))):
        B = _device_rhs(gpu, rng, 2, S.shape[0], False)
        Xd = U.linearSolveManyDevice_(fd, mode, None, B).cpu().numpy()
        Xh = U.linearSolveManyDevice_(fh, mode, M, B).cpu().numpy()
        assert fd.path == 5 and fh.path == 5
        assert np.array_equal(Xd, Xh)
        for c in range(2):
            assert _bwd(op, Xd[c], B[c].cpu().numpy()) <= 1e-13


@pytest.mark.parametrize("origin", ["host", "device"])
def test_two_threads_factor_from_one_handle_and_one_symbolic(gpu, pkg, origin, monkeypatch):
    """FEAST-style callers factor from several threads with one Symbolic: with a host-born one the first calls race to
    build its device pattern"""
    monkeypatch.setenv("SPL_LU_METHOD", "mf")
    U = pkg.umfpack
    S = _complex_shift(12)
    M = _mat(pkg, S)
    H = _handle(pkg, M)
    an = U.analyze(M) if origin == "host" else U.analyzeDevice(H)
    out = [None, None]

    def work(i):
        try:
            out[i] = U.factorDevice(H, an)
        except Exception as e:  # reported below
            out[i] = e

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not any(isinstance(o, Exception) for o in out), out
    single = U.factorDevice(H, an)
    B = _device_rhs(gpu, np.random.default_rng(6), 3, S.shape[0], True)
    want = U.linearSolveManyDevice_(single, U.UmfpackNormal, H, B).cpu().numpy()
    for f in out:
        assert f.path == single.path and f.stats == single.stats
        got = U.linearSolveManyDevice_(f, U.UmfpackNormal, H, B).cpu().numpy()
        assert np.array_equal(got.view(np.float64), want.view(np.float64))
    assert _bwd(S, want[0], B[0].cpu().numpy()) <= 1e-13


# ---- statuses --------------------------------------------------------------------------------------------------------------
def test_statuses(gpu, pkg, monkeypatch):
    import scipy.sparse as sp
    U = pkg.umfpack
    L = U._declare()
    S = _dominant_unsymmetric_grid(12)
    M = _mat(pkg, S)
    Mz = _mat(pkg, sp_csc(S * (1.0 + 0.5j)))
    H, Hz = _handle(pkg, M), _handle(pkg, Mz)
    an, anz = U.analyzeDevice(H), U.analyzeDevice(Hz)
    out = C.c_void_p()
    calls = [(L.spl_umfpack_di_symbolic_dev, L.spl_umfpack_di_numeric_dev, H, Hz, an, anz),
             (L.spl_umfpack_zi_symbolic_dev, L.spl_umfpack_zi_numeric_dev, Hz, H, anz, an)]
    for symbolic, numeric, mine, other, an_mine, an_other in calls:
        # UMFPACK_ERROR_argument_missing: no handle, not a matrix handle, no output pointer
        assert symbolic(None, C.byref(out)) == -5 and numeric(None, an_mine.value, C.byref(out)) == -5
        assert symbolic(an_mine.value, C.byref(out)) == -5 and numeric(an_mine.value, an_mine.value, C.byref(out)) == -5
        assert symbolic(mine.handle, None) == -5 and numeric(mine.handle, an_mine.value, None) == -5
        # UMFPACK_ERROR_invalid_matrix: a handle of the other value kind
        assert symbolic(other.handle, C.byref(out)) == -8 and numeric(other.handle, an_mine.value, C.byref(out)) == -8
        # UMFPACK_ERROR_invalid_Symbolic_object: none, not one, one of the other kind
        assert numeric(mine.handle, None, C.byref(out)) == -4
        assert numeric(mine.handle, mine.handle, C.byref(out)) == -4
        assert numeric(mine.handle, an_other.value, C.byref(out)) == -4
        assert out.value is None
    # UMFPACK_ERROR_invalid_matrix: handles without 32-bit row pointers (SPL_FORCE_PTR64=1 makes small ones)
    monkeypatch.setenv("SPL_FORCE_PTR64", "1")
    H64, Hz64 = _handle(pkg, M), _handle(pkg, Mz)
    monkeypatch.delenv("SPL_FORCE_PTR64")
    assert L.spl_umfpack_di_symbolic_dev(H64.handle, C.byref(out)) == -8
    assert L.spl_umfpack_di_numeric_dev(H64.handle, an.value, C.byref(out)) == -8
    assert L.spl_umfpack_zi_symbolic_dev(Hz64.handle, C.byref(out)) == -8
    assert L.spl_umfpack_zi_numeric_dev(Hz64.handle, anz.value, C.byref(out)) == -8
    assert out.value is None
    # UMFPACK_ERROR_invalid_matrix: a row block
    block = pkg.DeviceMatrix.from_csc(M, part=1, nparts=2)
    assert L.spl_umfpack_di_symbolic_dev(block.handle, C.byref(out)) == -8
    assert L.spl_umfpack_di_numeric_dev(block.handle, an.value, C.byref(out)) == -8
    # another shape than the analysed one
    small = _handle(pkg, _mat(pkg, _dominant_unsymmetric_grid(11)))
    assert L.spl_umfpack_di_numeric_dev(small.handle, an.value, C.byref(out)) == -11
    # a zero pivot: UMFPACK_WARNING_singular_matrix, as the host call
    Z = sp_csc(sp.csc_matrix(np.array([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 3.0]])))
    MZ = _mat(pkg, Z)
    HZ = _handle(pkg, MZ)
    fz = U.factorDevice(HZ, U.analyzeDevice(HZ))
    assert fz.status == 1 and U.factor(MZ, U.analyze(MZ)).status == 1
    # rectangular handles: the statuses of the host calls (analysed, "factored", refused by the solves)
    for cplx in (False, True):
        R = sp_csc(sp.csc_matrix(np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 4.0]])) * ((1.0 + 1.0j) if cplx else 1.0))
        ones = sp_csc(sp.csc_matrix(np.ones((3, 2))) * ((1.0 + 1.0j) if cplx else 1.0))
        for mat in (R, ones):
            MR = _mat(pkg, mat)
            HR = _handle(pkg, MR)
            fr_host = U.factor(MR, U.analyze(MR))
            for an_r in (U.analyzeDevice(HR), U.analyze(MR)):
                fr = U.factorDevice(HR, an_r)
                assert fr.status == fr_host.status
                with pytest.raises(U.UmfpackError) as e:
                    U.linearSolve_(fr, U.UmfpackNormal, MR, np.ones(3, dtype=np.complex128 if cplx else np.float64))
                assert e.value.status == -13
        assert U.factorDevice(_handle(pkg, _mat(pkg, ones)), U.analyze(_mat(pkg, ones))).status == 1


def test_complex_handle_whose_embedding_would_reach_2_31_entries(gpu, pkg):
    """UMFPACK_ERROR_out_of_memory, as embed() reports on the host route: 4 entries of the real embedding per stored
    complex entry, so from 2^29 stored entries on.  The handle is made on the device (7-point Laplacian on a 426^3
    grid: 540.1e6 entries, 11 GB as a complex handle); both calls refuse it on its size alone, before its pattern is
    exported or compared, so any `zi` Symbolic serves for the numeric call."""
    U = pkg.umfpack
    L = U._declare()
    m = 426
    R = pkg.DeviceMatrix.synthetic("poisson3d", m)
    Hz = R.to_complex()
    R.free()
    nnz = Hz.info()["nnz"]
    assert 2 ** 29 <= nnz < 2 ** 31 and Hz.is_complex
    out = C.c_void_p()
    assert L.spl_umfpack_zi_symbolic_dev(Hz.handle, C.byref(out)) == -1 and out.value is None
    small = _handle(pkg, _mat(pkg, _complex_unsymmetric_mesh(8)))
    an = U.analyzeDevice(small)
    assert L.spl_umfpack_zi_numeric_dev(Hz.handle, an.value, C.byref(out)) == -1 and out.value is None
    with pytest.raises(U.UmfpackError) as e:
        U.analyzeDevice(Hz)
    assert e.value.status == -1
    Hz.free()
    U.factorDevice(small, an)  # the Symbolic is unharmed

