"""LOBPCG on device handles (csrc/lobpcg.hip), real and complex.  The yardstick is the restatement of
tests/lobpcg_cases.py (checked on its own in tests/test_lobpcg_cpu.py); the device's values, vectors, residuals, history
and every count must equal it BIT FOR BIT, whatever the grid, the width of the inner products, the height of the
rotation's tile and the Gram tile are.  All comparisons are by view(uint64).  The Gram kernel and the rotation with a
complex Y, which the solver is built on, are pinned on their own in tests/test_gpu_gram.py."""
import ctypes as C

import numpy as np
import pytest

import amg_cases as AK
import krylov_cases as K
import lobpcg_cases as LK
from test_gpu_eigsh import dev, exported_levels, handle_of, host_columns, p_f64, p_i64

pytestmark = pytest.mark.gpu

KNOBS = ("SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH", "SPL_EIGSH_ROTATE_ROWS", "SPL_GRAM_TILE")
OK = 0


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


class Solver(object):
    """a LOBPCGSolver of the Python layer (which builds the preconditioner's parts) driven raw through its handle"""

    def __init__(self, pkg, torch, H, block, M=None):
        self.lib, self.torch = pkg._ffi.lib(), torch
        self.n, self.cplx, self.block = H.info()["nrows_global"], H.is_complex, block
        self.L = pkg.LOBPCGSolver(H, block, M)

    def solve(self, X0, nev, which=LK.SMALLEST, tol=1e-8, atol=0.0, max_iter=200):
        torch, n = self.torch, self.n
        ldx0, ldx = n + 1, n + 2
        dtype = np.complex128 if self.cplx else np.float64
        start = np.full(self.block * ldx0, np.nan, dtype=dtype)
        for j in range(self.block):
            start[j * ldx0:j * ldx0 + n] = X0[:, j]
        dX0 = dev(torch, start)
        dX = dev(torch, np.full(nev * ldx, np.nan, dtype=dtype))
        values, residuals = np.full(nev, 7.0), np.full(nev, 7.0)
        result, history = np.full(8, -1, dtype=np.int64), np.full(max_iter + 1, 7.0)
        st = self.lib.spl_lobpcg_solve_dev(self.L.handle, nev, which, tol, atol, max_iter, dX0.data_ptr(), ldx0, p_f64(values),
                                           dX.data_ptr(), ldx, p_f64(residuals), p_i64(result), p_f64(history),
                                           torch.cuda.current_stream().cuda_stream)
        assert st == OK, st
        reason, it, spmv, pairs, apps, sweeps, dropped, syncs = (int(v) for v in result)
        written = it + 1 if reason in (0, 1) else it  # the check that ends a solve writes its entry
        got = LK.Outcome(reason, it, spmv, apps, sweeps, dropped, syncs, values[:pairs], host_columns(dX, n, pairs, ldx),
                         residuals[:pairs], history[:written])
        got.untouched = (bool((values[pairs:] == 7.0).all()) and bool((residuals[pairs:] == 7.0).all())
                         and bool((history[written:] == 7.0).all())
                         and bool(np.isnan(dX.cpu().numpy().view(np.float64)[(2 if self.cplx else 1) * pairs * ldx:]).all())
                         and K.bits_equal(np.nan_to_num(dX0.cpu().numpy().view(np.float64), nan=5.0),
                                          np.nan_to_num(start.view(np.float64), nan=5.0)))
        return got

    def info(self):
        out = np.zeros(8, dtype=np.int64)
        assert self.lib.spl_lobpcg_info(self.L.handle, p_i64(out)) == OK
        return [int(v) for v in out]

    def free(self):
        self.L.free()


def same_outcome(got, want):
    assert got.result == want.result, (got.result, want.result)
    assert K.bits_equal(got.history, want.history), (got.history, want.history)
    assert K.bits_equal(got.values, want.values), (got.values, want.values)
    assert K.bits_equal(got.residuals, want.residuals), (got.residuals, want.residuals)
    assert got.vectors.shape == want.vectors.shape and K.bits_equal(got.vectors, want.vectors)
    assert got.untouched
    return True


def bytes_bound(n, block, vw):
    """the vectors, and above them the partials of the fold, the tables, the flags and the status block"""
    vectors = (7 * block + 1) * n * vw * 8
    chunks = -(-n // 4096)
    return vectors, vectors + 8 * 3 * block * vw * (chunks + 2) + 8 * (30 * block * block + 19 * block) + 12 * block + 64


@pytest.mark.parametrize("case", LK.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_solves_are_the_restatement(gpu, pkg, case):
    name, block, nev, which, tol, max_iter = case
    S = LK.matrix(name)
    want = LK.reference(*case)
    assert want.reason == (1 if name == "grid70" else 0) and want.pairs == nev
    L = Solver(pkg, gpu, handle_of(pkg, S), block)
    try:
        X0 = LK.start_of(name, block)
        assert same_outcome(L.solve(X0, nev, which, tol, 0.0, max_iter), want)
        # a second solve on the object: the same bits, and info counts it
        assert same_outcome(L.solve(X0, nev, which, tol, 0.0, max_iter), want)
        inf = L.info()
        vw = 2 if np.iscomplexobj(S.data) else 1
        low, high = bytes_bound(S.shape[0], block, vw)
        assert inf[:3] == [S.shape[0], block, vw - 1] and inf[4:6] == [2, want.iterations] and inf[6] > 0 and inf[7] == 0
        assert low <= inf[3] <= high, (low, inf[3], high)
    finally:
        L.free()
    if name in ("poisson12", "phased12") and which == LK.SMALLEST:  # both copies of the double lambda_2
        exact = np.linalg.eigvalsh(S.toarray())
        assert np.allclose(np.sort(want.values), exact[:4], rtol=0.0, atol=1e-9) and abs(exact[1] - exact[2]) < 1e-12


@pytest.mark.parametrize("kind,block,nev,tol,max_iter", LK.PRECONDITIONED)
def test_preconditioned_solves_are_the_restatement(gpu, pkg, kind, block, nev, tol, max_iter):
    S = LK.matrix("poisson8")
    H = handle_of(pkg, S)
    owned = None
    if kind == "amg":
        owned = H.amg(coarse_size=16)
        assert owned.levels >= 2
        M_dev, M_ref = owned, AK.Cycle(exported_levels(owned), 1, 4)
    elif kind == "ilu0":
        owned = H.ilu0()
        M_dev, M_ref = owned, K.preconditioner(S, "ilu0")
    else:
        M_dev, M_ref = kind, K.preconditioner(S, kind)
    X0 = LK.start_of("poisson8", block)
    want = LK.lobpcg(S, X0, nev, LK.SMALLEST, tol, 0.0, max_iter, M_ref)
    assert want.reason == 0 and want.applications == block * want.iterations
    exact = np.linalg.eigvalsh(S.toarray())
    assert np.allclose(np.sort(want.values), exact[:nev], rtol=0.0, atol=1e-7)
    L = Solver(pkg, gpu, H, block, M_dev)
    try:
        assert same_outcome(L.solve(X0, nev, LK.SMALLEST, tol, 0.0, max_iter), want)
        assert L.info()[2] == {"jacobi": 4, "sgs": 2 | 4 | 8, "ilu0": 2 | 8, "amg": 16}[kind]
    finally:
        L.free()
        if owned is not None:
            owned.free()


def test_knobs_do_not_show_in_a_solve(gpu, pkg, monkeypatch):
    for case in (("poisson12", 6, 4, LK.SMALLEST, 1e-9, 200), ("phased12", 6, 4, LK.SMALLEST, 1e-9, 200),
                 ("grid70", 4, 2, LK.SMALLEST, 1e-9, 3)):
        S = LK.matrix(case[0])
        want = LK.reference(*case)
        L = Solver(pkg, gpu, handle_of(pkg, S), case[1])
        try:
            for grid, batch, rows, tile in (("1", "2", "16", "1"), ("3", "8", "64", "4"), ("7", "4", "32", "2")):
                for name, value in zip(KNOBS, (grid, batch, rows, tile)):
                    monkeypatch.setenv(name, value)
                assert same_outcome(L.solve(LK.start_of(case[0], case[1]), case[2], case[3], case[4], 0.0, case[5]), want)
        finally:
            L.free()


def test_outcomes_of_the_header(gpu, pkg):
    D = LK.matrix("diagonal")
    L = Solver(pkg, gpu, handle_of(pkg, D), 3)
    try:
        # unit vectors on a diagonal matrix: R = 0, converged at iteration 0
        X0 = np.eye(8)[:, :3]
        got = L.solve(X0, 2, LK.SMALLEST, 1e-10, 0.0, 50)
        assert got.result == [0, 0, 5, 2, 0, 0, 0, 4] and list(got.values) == [1.0, 2.0] and list(got.residuals) == [0.0, 0.0]
        assert same_outcome(got, LK.lobpcg(D, X0, 2, LK.SMALLEST, 1e-10, 0.0, 50))
        # a repeated column: the start block is rank deficient
        X0 = LK.start_block(8, 3)
        X0[:, 2] = X0[:, 0]
        got = L.solve(X0, 2)
        assert got.result == [2, 0, 0, 0, 0, 0, 0, 1] and same_outcome(got, LK.lobpcg(D, X0, 2))
        # a NaN in the start block
        X0 = LK.start_block(8, 3)
        X0[4, 1] = np.nan
        got = L.solve(X0, 2)
        assert got.result == [3, 0, 0, 0, 0, 0, 0, 1] and got.untouched
        # max_iter = 0: the check of iteration 0 ends it, with the pairs of the start's Rayleigh-Ritz
        X0 = LK.start_block(8, 3)
        got = L.solve(X0, 2, LK.LARGEST, 1e-10, 0.0, 0)
        assert got.reason == 1 and got.iterations == 0 and got.pairs == 2
        assert same_outcome(got, LK.lobpcg(D, X0, 2, LK.LARGEST, 1e-10, 0.0, 0))
        assert L.info()[4] == 4
    finally:
        L.free()


def test_the_python_layer(gpu, pkg):
    S = LK.matrix("poisson12")
    want = LK.reference("poisson12", 6, 4, LK.SMALLEST, 1e-9, 200)
    H = handle_of(pkg, S)
    X0 = LK.start_of("poisson12", 6)
    values, vectors, res = H.lobpcg(X0, nev=4, tol=1e-9)  # host arrays
    assert res["converged"] and res["iterations"] == want.iterations and res["pairs"] == 4
    assert K.bits_equal(values, want.values) and K.bits_equal(np.ascontiguousarray(vectors), want.vectors)
    assert K.bits_equal(res["residuals"], want.residuals) and K.bits_equal(res["history"], want.history)
    values, vectors, res = H.lobpcg(gpu.from_numpy(X0).cuda(), nev=4, tol=1e-9)  # a device tensor
    assert K.bits_equal(values, want.values) and K.bits_equal(np.ascontiguousarray(vectors.cpu().numpy()), want.vectors)
    host = pkg.Matrix(S.shape[1], S.shape[0], S.tocsc().indptr, S.tocsc().indices, S.tocsc().data)
    values, _, res = pkg.lobpcg(host, X0, nev=4, tol=1e-9)
    assert K.bits_equal(values, want.values) and res["reason_name"] == "converged"
