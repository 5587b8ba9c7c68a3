"""LOBPCG with a mass matrix on device handles (spl_lobpcg_set_mass, csrc/lobpcg.hip), real and complex.  The yardstick is
the restatement of tests/globpcg_cases.py (checked on its own in tests/test_globpcg_cpu.py): the device's values, vectors,
residuals, history and every count must equal it BIT FOR BIT, whatever the grid, the width of the inner products, the
height of the rotation's tile and the Gram tile are.  With an identity handle for B the solve must equal the standard
solve of the same object.  The paired update the method is built on is pinned on its own in tests/test_gpu_update_pair.py.

A B with a NaN entry never reaches a solve: spl_matrix_hermitian says 0 for it (IEEE ==), so spl_lobpcg_set_mass refuses
it with SPL_ERROR_invalid_matrix, as the header's error list says.  Reason 3 through the mass matrix is reached with an
entry of +Inf instead, which passes the Hermitian test and makes B X not finite."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as AK
import globpcg_cases as GK
import krylov_cases as K
import lobpcg_cases as LK
from test_gpu_eigsh import exported_levels, handle_of
from test_gpu_lobpcg import KNOBS, Solver, same_outcome

pytestmark = pytest.mark.gpu

MATRIX = -8  # SPL_ERROR_invalid_matrix


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def with_mass(pkg, torch, S, Bm, block, M=None):
    """a Solver of tests/test_gpu_lobpcg.py on S with the mass matrix Bm (a scipy matrix or a DeviceMatrix)"""
    L = Solver(pkg, torch, handle_of(pkg, S) if sp.issparse(S) else S, block, M)
    L.L.set_mass(Bm if isinstance(Bm, pkg.DeviceMatrix) else handle_of(pkg, Bm))
    return L


def same_generalized_outcome(L, got, want):
    assert same_outcome(got, want)
    inf = L.L.info()
    assert inf["generalized"] and inf["flags"] & 32 and inf["mass_columns"] == want.mass_columns, (inf, want.mass_columns)
    return True


def mass_bytes(n, block, vw):
    return (3 * block + 1) * n * vw * 8


@pytest.mark.parametrize("case", GK.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_solves_are_the_restatement(gpu, pkg, case):
    name, bname, block, nev, which, tol, max_iter = case
    S, Bm = LK.matrix(name), GK.mass(bname)
    want = GK.reference(*case)
    assert want.reason == (1 if name == "grid70" else 0) and want.pairs == nev
    L = Solver(pkg, gpu, handle_of(pkg, S), block)
    try:
        plain_bytes = L.L.info()["device_bytes"]
        L.L.set_mass(handle_of(pkg, Bm))
        X0 = LK.start_of(name, block)
        assert same_generalized_outcome(L, L.solve(X0, nev, which, tol, 0.0, max_iter), want)
        # a second solve on the object: the same bits, and info counts it
        assert same_generalized_outcome(L, L.solve(X0, nev, which, tol, 0.0, max_iter), want)
        inf = L.info()
        vw = 2 if np.iscomplexobj(S.data) else 1
        assert inf[:3] == [S.shape[0], block, (vw - 1) | 32] and inf[4:6] == [2, want.iterations] and inf[6] > 0
        assert inf[7] == want.mass_columns
        assert inf[3] == plain_bytes + mass_bytes(S.shape[0], block, vw)  # 10 block + 2 vectors in all
    finally:
        L.free()


@pytest.mark.parametrize("kind,block,nev,tol,max_iter", GK.PRECONDITIONED)
def test_preconditioned_solves_are_the_restatement(gpu, pkg, kind, block, nev, tol, max_iter):
    S, Bm = LK.matrix("poisson8"), GK.mass("mass8_3d")
    H = handle_of(pkg, S)
    owned = None
    if kind == "amg":
        owned = H.amg(coarse_size=16)
        assert owned.levels >= 2
        M_dev, M_ref = owned, AK.Cycle(exported_levels(owned), 1, 4)
    else:
        M_dev, M_ref = kind, K.preconditioner(S, kind)
    X0 = LK.start_of("poisson8", block)
    want = GK.lobpcg(S, Bm, X0, nev, LK.SMALLEST, tol, 0.0, max_iter, M_ref)
    assert want.reason == 0 and want.applications == block * want.iterations
    L = with_mass(pkg, gpu, H, Bm, block, M_dev)
    try:
        assert same_generalized_outcome(L, L.solve(X0, nev, LK.SMALLEST, tol, 0.0, max_iter), want)
        assert L.info()[2] == {"jacobi": 4, "amg": 16}[kind] | 32
    finally:
        L.free()
        if owned is not None:
            owned.free()


@pytest.mark.parametrize("name", ["poisson12", "phased12"])
def test_an_identity_handle_gives_the_standard_solve(gpu, pkg, name):
    S = LK.matrix(name)
    cplx = np.iscomplexobj(S.data)
    n, block, nev = S.shape[0], 6, 4
    X0 = LK.start_of(name, block)
    ones = gpu.ones(n, dtype=gpu.complex128 if cplx else gpu.float64, device="cuda")
    I = pkg.DeviceMatrix.diag_dev(n, ones.data_ptr(), cplx)  # spl_matrix_diag_dev of ones
    L = Solver(pkg, gpu, handle_of(pkg, S), block)
    try:
        before = L.solve(X0, nev, LK.SMALLEST, 1e-9, 0.0, 200)
        assert same_outcome(before, LK.reference(name, block, nev, LK.SMALLEST, 1e-9, 200))
        plain = L.L.info()
        L.L.set_mass(I)
        got = L.solve(X0, nev, LK.SMALLEST, 1e-9, 0.0, 200)
        assert got.result == before.result and got.untouched
        assert np.array_equal(got.values, before.values) and np.array_equal(got.vectors, before.vectors)
        assert np.array_equal(got.residuals, before.residuals) and np.array_equal(got.history, before.history)
        inf = L.L.info()
        assert inf["generalized"] and inf["mass_columns"] == block + block * before.iterations + nev
        assert inf["device_bytes"] == plain["device_bytes"] + mass_bytes(n, block, 2 if cplx else 1)
        L.L.set_mass(None)  # the standard method, its memory and its bits are back
        again = L.solve(X0, nev, LK.SMALLEST, 1e-9, 0.0, 200)
        assert same_outcome(again, LK.reference(name, block, nev, LK.SMALLEST, 1e-9, 200))
        inf = L.L.info()
        assert not inf["generalized"] and inf["mass_columns"] == 0 and inf["flags"] == plain["flags"]
        assert inf["device_bytes"] == plain["device_bytes"]
    finally:
        L.free()


def test_knobs_do_not_show_in_a_solve(gpu, pkg, monkeypatch):
    for case in (("poisson12", "mass12", 6, 4, LK.SMALLEST, 1e-9, 200), ("phased12", "phased_mass12", 6, 4, LK.SMALLEST, 1e-9, 200),
                 ("grid70", "mass70", 4, 2, LK.SMALLEST, 1e-9, 3)):
        name, bname, block, nev, which, tol, max_iter = case
        want = GK.reference(*case)
        L = with_mass(pkg, gpu, LK.matrix(name), GK.mass(bname), block)
        try:
            for grid, batch, rows, tile in (("1", "2", "16", "1"), ("3", "8", "64", "4"), ("7", "4", "32", "2")):
                for knob, value in zip(KNOBS, (grid, batch, rows, tile)):
                    monkeypatch.setenv(knob, value)
                assert same_generalized_outcome(L, L.solve(LK.start_of(name, block), nev, which, tol, 0.0, max_iter), want)
        finally:
            L.free()


def diagonal_mass():
    return LK._csr(sp.diags([np.array([1.0, 2.0, 2.0, 2.0, 1.0, 1.0, 2.0, 1.0])], [0]))


def test_outcomes_of_the_header(gpu, pkg):
    D = LK.matrix("diagonal")
    Bm = diagonal_mass()
    L = with_mass(pkg, gpu, D, Bm, 3)
    try:
        # a repeated column: the start block is rank deficient in the inner product of B too
        X0 = LK.start_block(8, 3)
        X0[:, 2] = X0[:, 0]
        got = L.solve(X0, 2)
        assert got.result == [2, 0, 0, 0, 0, 0, 0, 1] and same_generalized_outcome(L, got, GK.lobpcg(D, Bm, X0, 2))
        assert L.L.info()["mass_columns"] == 3  # B X was formed
        # B = -I: every q0 < 0, so every start column drops
        minus = gpu.full((8,), -1.0, dtype=gpu.float64, device="cuda")
        L.L.set_mass(pkg.DeviceMatrix.diag_dev(8, minus.data_ptr()))
        X0 = LK.start_block(8, 3)
        got = L.solve(X0, 2)
        assert got.result == [2, 0, 0, 0, 0, 0, 0, 1]
        assert same_generalized_outcome(L, got, GK.lobpcg(D, LK._csr(-sp.identity(8)), X0, 2))
        # a NaN entry: refused by set_mass (the Hermitian test is IEEE ==), and the mass matrix stays what it was
        bad = Bm.copy()
        bad.data[3] = np.nan
        with pytest.raises(pkg._ffi.SparseLinearError) as refused:
            L.L.set_mass(handle_of(pkg, bad))
        assert refused.value.status == MATRIX
        assert L.solve(X0, 2).result == [2, 0, 0, 0, 0, 0, 0, 1]  # still -I
        # an entry of +Inf passes that test; B X is not finite: reason 3
        bad = Bm.copy()
        bad.data[3] = np.inf
        L.L.set_mass(handle_of(pkg, bad))
        got = L.solve(X0, 2)
        assert got.result == [3, 0, 0, 0, 0, 0, 0, 1] and got.untouched
        assert same_generalized_outcome(L, got, GK.lobpcg(D, bad, X0, 2))
    finally:
        L.free()
    # a zero column of W: x_0 = e_0 is an exact eigenvector, so r_0 = 0, and its column of W drops and is counted
    L = with_mass(pkg, gpu, D, Bm, 2)
    try:
        X0 = np.zeros((8, 2))
        X0[0, 0] = 1.0
        X0[1:4, 1] = [1.0, 0.5, 0.25]
        want = GK.lobpcg(D, Bm, X0, 2, LK.SMALLEST, 1e-10, 0.0, 50)
        assert want.reason == 0 and want.dropped >= 1 and want.residuals[0] == 0.0
        got = L.solve(X0, 2, LK.SMALLEST, 1e-10, 0.0, 50)
        assert got.result[6] == want.dropped and same_generalized_outcome(L, got, want)
    finally:
        L.free()


def test_the_python_layer(gpu, pkg):
    S, Bm = LK.matrix("poisson12"), GK.mass("mass12")
    want = GK.reference("poisson12", "mass12", 6, 4, LK.SMALLEST, 1e-9, 200)
    H, HB = handle_of(pkg, S), handle_of(pkg, Bm)
    X0 = LK.start_of("poisson12", 6)
    values, vectors, res = H.lobpcg(X0, nev=4, tol=1e-9, B=HB)  # host arrays
    assert res["converged"] and res["iterations"] == want.iterations and res["pairs"] == 4
    assert K.bits_equal(values, want.values) and K.bits_equal(np.ascontiguousarray(vectors), want.vectors)
    assert K.bits_equal(res["residuals"], want.residuals) and K.bits_equal(res["history"], want.history)
    values, vectors, res = H.lobpcg(gpu.from_numpy(X0).cuda(), nev=4, tol=1e-9, B=HB)  # a device tensor
    assert K.bits_equal(values, want.values) and K.bits_equal(np.ascontiguousarray(vectors.cpu().numpy()), want.vectors)
    L = pkg.LOBPCGSolver(H, 6, None, HB)  # the constructor's keyword, and the object keeps B
    try:
        assert L.B is HB and L.info()["generalized"] and L.info()["mass_columns"] == 0
        values, _, res = L.solve(X0, 4, tol=1e-9)
        assert K.bits_equal(values, want.values) and L.info()["mass_columns"] == want.mass_columns
        L.set_mass(None)
        assert L.B is None and not L.info()["generalized"]
        with pytest.raises(ValueError):
            L.set_mass(Bm)  # a scipy matrix is no DeviceMatrix
    finally:
        L.free()

    def host(M):
        return pkg.Matrix(M.shape[1], M.shape[0], M.tocsc().indptr, M.tocsc().indices, M.tocsc().data)

    values, _, res = pkg.lobpcg(host(S), X0, nev=4, tol=1e-9, B=host(Bm))
    assert K.bits_equal(values, want.values) and res["reason_name"] == "converged"
