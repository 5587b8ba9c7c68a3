"""Thick-restart Lanczos on device handles and its in-place basis rotation (csrc/eigsh.hip), real and complex.  The
yardstick is the restatement of tests/eigsh_cases.py (checked on its own in tests/test_eigsh_cpu.py); the device's rotated
columns, values, vectors, residuals, histories and counts must equal it BIT FOR BIT, whatever the grid, the width of the
inner products and the height of the rotation's tile are.  All comparisons are by view(uint64)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as AK
import eigsh_cases as EK
import krylov_cases as K

pytestmark = pytest.mark.gpu

KNOBS = ("SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH", "SPL_EIGSH_ROTATE_ROWS")
BOTH = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
SHAPES = ((1, 1), (2, 1), (3, 2), (64, 63), (127, 5), (128, 127), (128, 128))
OK, HANDLE, MISSING, NONPOSITIVE, MATRIX, MISMATCH, OVERFLOW = 0, -3, -5, -6, -8, -20, -22


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def handle_of(pkg, S):
    """a whole device handle with the entries of the scipy matrix S (explicit zeros included), real or complex"""
    S = sp.csc_matrix(S)
    S.sort_indices()
    M = pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)
    return pkg.DeviceMatrix.from_csc_complex(M) if np.iscomplexobj(S.data) else pkg.DeviceMatrix.from_csc(M)


def scipy_of(H):
    inf = H.info()
    rp, ci, v = H.export_csr()
    return sp.csr_matrix((v, ci, rp), shape=(inf["nrows_global"], inf["ncols"]))


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the cached inputs are read-only


def p_f64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def p_i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


# ---- 1. the rotation -------------------------------------------------------------------------------------------------------
_rotation = {}


def rotation_case(n, m, k, cplx):
    """V (n x m), Y (m x k) and the restated V Y, computed once; values whose bits matter among ordinary numbers"""
    key = (n, m, k, cplx)
    if key not in _rotation:
        rng = np.random.default_rng(1000 * m + k + n + cplx)
        V = rng.standard_normal((n, m))
        if cplx:
            V = V + 1j * rng.standard_normal((n, m))
        V[0, 0] = -0.0
        if n > 2:
            V[1, m - 1], V[2, 0] = 5e-324, 1e300
        Y = rng.standard_normal((m, k))
        Y[m - 1, k - 1] = -0.0
        want = EK.rotate(V, Y)
        for a in (V, Y, want):
            a.setflags(write=False)
        _rotation[key] = (V, Y, want)
    return _rotation[key]


def device_columns(torch, A, ld, fill=np.nan):
    """the columns of A one after the other, ld entries apart, the gaps filled (nothing may read or write them)"""
    n, cols = A.shape
    out = np.full(max(cols * ld, 1), fill, dtype=A.dtype)
    for i in range(cols):
        out[i * ld:i * ld + n] = A[:, i]
    return dev(torch, out)


def host_columns(t, n, cols, ld):
    a = t.cpu().numpy()
    return np.stack([a[i * ld:i * ld + n] for i in range(cols)], axis=1) if cols else np.zeros((n, 0), dtype=a.dtype)


def raw_rotate(pkg, torch, n, m, k, dV, ldv, dY, ldy, dout, ldo, cplx):
    st = pkg._ffi.lib().spl_vector_rotate_dev(n, 2 if cplx else 1, m, k, dV.data_ptr(), ldv, dY.data_ptr(), ldy,
                                              dout.data_ptr() if dout is not None else None, ldo,
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def same_with_nan_gaps(got, want):
    """bit for bit where `want` is a number, NaN where it is NaN"""
    g, w = np.ascontiguousarray(got).view(np.float64), np.ascontiguousarray(want).view(np.float64)
    gaps = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), gaps) and K.bits_equal(g[~gaps], w[~gaps])


def check_rotation(pkg, torch, n, m, k, cplx, ldv, ldy, ldo):
    V, Y, want = rotation_case(n, m, k, cplx)
    dY = device_columns(torch, Y, ldy)
    # beside V
    dV = device_columns(torch, V, ldv)
    before = dV.cpu().numpy()
    dout = device_columns(torch, np.full((n, k), 7.0, dtype=V.dtype), ldo)
    assert raw_rotate(pkg, torch, n, m, k, dV, ldv, dY, ldy, dout, ldo, cplx) == OK
    assert K.bits_equal(host_columns(dout, n, k, ldo), want), (n, m, k, "out")
    assert same_with_nan_gaps(dV.cpu().numpy(), before), "V is untouched"
    expect = device_columns(torch, want, ldo).cpu().numpy()
    assert same_with_nan_gaps(dout.cpu().numpy(), expect), "the rows beyond n are untouched"
    # in place
    assert raw_rotate(pkg, torch, n, m, k, dV, ldv, dY, ldy, None, 0, cplx) == OK
    after = before.copy()
    for i in range(k):
        after[i * ldv:i * ldv + n] = want[:, i]
    assert same_with_nan_gaps(dV.cpu().numpy(), after), (n, m, k, "in place: columns k ... and the rows beyond n stay")


@BOTH
@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5])
def test_rotation_is_the_restatement(gpu, pkg, n, cplx):
    for m, k in SHAPES:
        check_rotation(pkg, gpu, n, m, k, cplx, n + 3, m + 2, n + 1)
    check_rotation(pkg, gpu, n, 3, 2, cplx, n, 3, n)


@BOTH
def test_rotation_knobs_do_not_show(gpu, pkg, monkeypatch, cplx):
    for rows in ("16", "32", "64", "5", None):
        for grid in ("1", "3", None):
            for name, value in (("SPL_EIGSH_ROTATE_ROWS", rows), ("SPL_KRYLOV_GRID", grid)):
                if value is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, value)
            for n in (33, 4097):
                for m, k in ((3, 2), (64, 63), (128, 128)):
                    check_rotation(pkg, gpu, n, m, k, cplx, n + 3, m + 2, n + 1)


def test_rotation_of_nothing_and_the_error_order(gpu, pkg):
    lib = pkg._ffi.lib()
    V = gpu.full((64,), 3.0, dtype=gpu.float64, device="cuda")
    Y = gpu.ones(16, dtype=gpu.float64, device="cuda")
    out = gpu.full((64,), 5.0, dtype=gpu.float64, device="cuda")

    def call(n=4, vw=1, m=2, k=1, v=V.data_ptr(), ldv=8, y=Y.data_ptr(), ldy=4, o=out.data_ptr(), ldo=8):
        return lib.spl_vector_rotate_dev(n, vw, m, k, v, ldv, y, ldy, o, ldo, None)

    assert call(n=0) == OK and call(n=0, v=None, y=None, o=None) == OK
    gpu.cuda.synchronize()
    assert bool((V == 3.0).all()) and bool((out == 5.0).all())
    assert call(n=-1, vw=3) == NONPOSITIVE
    for bad in (dict(vw=0), dict(vw=3), dict(m=0), dict(m=129), dict(k=0), dict(k=3), dict(ldv=3), dict(ldy=1), dict(ldo=3),
                dict(v=None), dict(y=None), dict(vw=2, v=V.data_ptr() + 8), dict(y=Y.data_ptr() + 4),
                dict(vw=2, o=out.data_ptr() + 8), dict(o=V.data_ptr()), dict(o=V.data_ptr() + 8 * 11),
                dict(k=2, v=V.data_ptr() + 8 * 8, o=V.data_ptr(), ldo=60)):
        assert call(**bad) == MISSING, bad
    assert call(o=V.data_ptr() + 8 * 12) == OK  # right behind V's last entry
    assert call(o=None, ldo=0) == OK
    gpu.cuda.synchronize()


# ---- 2. the solver -----------------------------------------------------------------------------------------------------------
class Raw(object):
    """the raw calls on a handle: create, set_inverse, solve_dev, info, free"""

    def __init__(self, pkg, torch, H, ncv):
        self.lib, self.torch, self.H = pkg._ffi.lib(), torch, H
        self.n, self.cplx = H.info()["nrows_global"], H.is_complex
        self.e = C.c_void_p()
        self.status = self.lib.spl_eigsh_create(H.handle, ncv, C.byref(self.e))

    def set_inverse(self, solver, sigma, rtol=EK.INNER_RTOL, atol=0.0, max_iter=EK.INNER_MAXITER):
        return self.lib.spl_eigsh_set_inverse(self.e, solver.handle if solver is not None else None, sigma, rtol, atol,
                                              max_iter)

    def solve(self, v0, nev, which, tol=1e-10, atol=0.0, max_restarts=200, ldx=None):
        torch = self.torch
        ldx = self.n + 2 if ldx is None else ldx
        dv0 = dev(torch, v0)
        dtype = np.complex128 if self.cplx else np.float64
        dX = dev(torch, np.full(nev * ldx, np.nan, dtype=dtype))
        values, residuals = np.full(nev, 7.0), np.full(nev, 7.0)
        result, history = np.full(6, -1, dtype=np.int64), np.full(max_restarts + 1, 7.0)
        st = self.lib.spl_eigsh_solve_dev(self.e, nev, EK.WHICH[which], tol, atol, max_restarts, dv0.data_ptr(),
                                          p_f64(values), dX.data_ptr(), ldx, p_f64(residuals), p_i64(result),
                                          p_f64(history), torch.cuda.current_stream().cuda_stream)
        assert st == OK, st
        pairs, cycles = int(result[3]), int(result[1])
        got = EK.Outcome(int(result[0]), cycles, int(result[2]), values[:pairs], host_columns(dX, self.n, pairs, ldx),
                         residuals[:pairs], history[:cycles + 1], int(result[4]), int(result[5]), ())
        got.untouched = (bool((values[pairs:] == 7.0).all()) and bool((residuals[pairs:] == 7.0).all())
                         and bool((history[cycles + 1:] == 7.0).all())
                         and bool(np.isnan(dX.cpu().numpy().view(np.float64)[2 * pairs * ldx if self.cplx else pairs * ldx:])
                                  .all()))
        return got

    def info(self):
        out = np.zeros(8, dtype=np.int64)
        assert self.lib.spl_eigsh_info(self.e, p_i64(out)) == OK
        return [int(v) for v in out]

    def free(self):
        self.lib.spl_eigsh_free(C.byref(self.e))


def same_outcome(got, want):
    assert got.result == want.result, (got.result, want.result)
    assert K.bits_equal(got.history, want.history), (got.history, want.history)
    assert K.bits_equal(got.values, want.values), (got.values, want.values)
    assert K.bits_equal(got.residuals, want.residuals), (got.residuals, want.residuals)
    assert got.vectors.shape == want.vectors.shape and K.bits_equal(got.vectors, want.vectors)
    assert got.untouched
    return True


def start_of(S):
    return EK.start_vector(S.shape[0], np.iscomplexobj(S.data))


def grid_handle(pkg):
    """the anisotropic 5 x 6 x 7 grid assembled on the device with `kronecker` and `lin`"""
    L = [handle_of(pkg, EK.laplacian(m)) for m in (5, 6, 7)]
    I = [pkg.DeviceMatrix.ident(m) for m in (5, 6, 7)]
    terms = (L[0].kronecker(I[1]).kronecker(I[2]), I[0].kronecker(L[1]).kronecker(I[2]),
             I[0].kronecker(I[1]).kronecker(L[2]))
    H = terms[0].lin(1.0, terms[1], 1.3).lin(1.0, terms[2], 1.7)
    want, got = EK.matrix("grid"), scipy_of(H)
    got.sort_indices()
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data, want.data), "the device's assembly is the restatement's matrix"
    return H


@pytest.mark.parametrize("case", EK.DIRECT, ids=lambda c: "-".join(str(v) for v in c))
def test_direct_solves_are_the_restatement(gpu, pkg, case):
    name, which, nev, ncv, tol, max_restarts = case
    S = EK.matrix(name)
    want = EK.reference(*case)
    assert want.reason == 0
    H = grid_handle(pkg) if name == "grid" else handle_of(pkg, S)
    E = Raw(pkg, gpu, H, ncv)
    assert E.status == OK
    try:
        assert same_outcome(E.solve(start_of(S), nev, which, tol, 0.0, max_restarts), want)
        inf = E.info()
        assert inf[:3] == [S.shape[0], ncv, 1 if np.iscomplexobj(S.data) else 0] and inf[4:6] == [1, want.cycles]
        assert inf[3] >= (ncv + 2) * S.shape[0] * (16 if np.iscomplexobj(S.data) else 8) and inf[6] > 0 and inf[7] == 0
    finally:
        E.free()


def exported_levels(M):
    levels = []
    for l in range(M.levels):
        got = M.level(l)
        levels.append(AK.Level(scipy_of(got["A"]), got["w"].cpu().numpy(), None if got["P"] is None else scipy_of(got["P"]),
                               None if got["R"] is None else scipy_of(got["R"])))
    return levels


@pytest.mark.parametrize("sigma,kind,nev,ncv", EK.INVERSE)
def test_inverse_solves_are_the_restatement(gpu, pkg, sigma, kind, nev, ncv):
    S = EK.matrix("grid")
    H = handle_of(pkg, S)
    Hs = handle_of(pkg, EK.shifted(S, sigma))
    amg = Hs.amg(coarse_size=16) if kind == "amg" else None
    M = AK.Cycle(exported_levels(amg), 1, 4) if kind == "amg" else kind
    if kind == "amg":
        assert amg.levels >= 2
    want = EK.inverse_reference(sigma, M, nev, ncv)
    assert want.reason == 0 and want.inner > 0 and want.pairs == nev
    exact = np.linalg.eigvalsh(S.toarray())
    nearest = exact[np.argsort(np.abs(exact - sigma), kind="stable")][:nev]
    assert np.allclose(want.values, nearest, rtol=0.0, atol=1e-9)
    solver = pkg.KrylovSolver(Hs, "cg", amg if kind == "amg" else kind)
    E = Raw(pkg, gpu, H, ncv)
    try:
        assert E.set_inverse(solver, sigma) == OK and E.info()[2] == 2
        assert same_outcome(E.solve(start_of(S), nev, "LM"), want)
        assert E.set_inverse(None, 0.0) == OK and E.info()[2] == 0  # back to A itself
    finally:
        E.free()
        solver.free()
        if amg is not None:
            amg.free()


def test_knobs_do_not_show_in_a_solve(gpu, pkg, monkeypatch):
    for case in (("ramp", "SA", 3, 12, 1e-10, 200), ("hermitian", "LA", 3, 16, 1e-10, 200),
                 ("banded", "LA", 4, 12, 1e-8, 50)):
        S = EK.matrix(case[0])
        want = EK.reference(*case)
        E = Raw(pkg, gpu, handle_of(pkg, S), case[3])
        try:
            for grid, batch, rows in (("1", "2", "16"), ("3", "8", "64"), ("7", "4", "32")):
                monkeypatch.setenv("SPL_KRYLOV_GRID", grid)
                monkeypatch.setenv("SPL_GMRES_DOTS_BATCH", batch)
                monkeypatch.setenv("SPL_EIGSH_ROTATE_ROWS", rows)
                assert same_outcome(E.solve(start_of(S), case[2], case[1], case[4], 0.0, case[5]), want), (grid, batch, rows)
        finally:
            E.free()


# ---- 3. the outcomes -----------------------------------------------------------------------------------------------------------
def test_invariant_subspaces_and_a_zero_start(gpu, pkg):
    two = sp.csr_matrix(2.0 * sp.identity(16))
    ones = np.ones(16)  # v_0 = 1/4 in every entry: <v_0,v_0> is 1 exactly, and w - 2 v_0 is 0 exactly
    E = Raw(pkg, gpu, handle_of(pkg, two), 4)
    try:
        got = E.solve(ones, 1, "LA")
        assert got.result == [0, 1, 1, 1, 0, 0] and got.values[0] == 2.0 and got.residuals[0] == 0.0
        assert same_outcome(got, EK.eigsh(two, ones, 1, "LA", 4))
        got = E.solve(ones, 2, "LA")
        assert got.result[0] == 2 and got.pairs == 1
        assert same_outcome(got, EK.eigsh(two, ones, 2, "LA", 4))
        got = E.solve(np.zeros(16), 2, "LA")
        assert got.result == [2, 0, 0, 0, 0, 0] and got.history[0] == 0.0 and got.untouched
        assert E.info()[4] == 3
    finally:
        E.free()
    D = sp.csr_matrix(sp.diags([np.arange(1.0, 7.0)], [0]))
    e1 = np.zeros(6)
    e1[0] = 1.0
    E = Raw(pkg, gpu, handle_of(pkg, D), 4)
    try:
        got = E.solve(e1, 1, "LA")
        assert got.result[:4] == [0, 1, 1, 1] and got.values[0] == 1.0  # eta == 0 closed the first cycle
        assert same_outcome(got, EK.eigsh(D, e1, 1, "LA", 4))
    finally:
        E.free()


def test_not_finite_is_reason_3_and_a_nan_matrix_is_refused(gpu, pkg):
    bad = sp.csr_matrix(sp.diags([[1.0, np.inf, 3.0, 4.0, 5.0, 6.0]], [0]))
    v0 = EK.start_vector(6)
    E = Raw(pkg, gpu, handle_of(pkg, bad), 4)
    try:
        assert E.status == OK
        got = E.solve(v0, 1, "LA")
        assert got.result == [3, 0, 1, 0, 0, 0] and got.untouched
        assert same_outcome(got, EK.eigsh(bad, v0, 1, "LA", 4))
        got = E.solve(np.array([1.0, np.inf, 0.0, 0.0, 0.0, 0.0]), 1, "LA")
        assert got.result == [3, 0, 0, 0, 0, 0] and got.history[0] == np.inf
    finally:
        E.free()
    nan = sp.csr_matrix(sp.diags([[1.0, np.nan, 3.0, 4.0, 5.0, 6.0]], [0]))
    E = Raw(pkg, gpu, handle_of(pkg, nan), 4)
    assert E.status == MATRIX and not E.e.value


def test_max_restarts_is_reason_1_with_the_restatement_s_pairs(gpu, pkg):
    case = ("ramp", "SA", 3, 12, 1e-10, 1)
    want = EK.reference(*case)
    assert want.reason == 1 and want.pairs == 3
    S = EK.matrix("ramp")
    E = Raw(pkg, gpu, handle_of(pkg, S), 12)
    try:
        assert same_outcome(E.solve(start_of(S), 3, "SA", 1e-10, 0.0, 1), want)
        # a second solve on the object: the same bits, and info counts it
        assert same_outcome(E.solve(start_of(S), 3, "SA", 1e-10, 0.0, 1), want)
        assert E.info()[4:6] == [2, 1]
    finally:
        E.free()
        E.free()  # idempotent
        assert not E.e.value
    pkg._ffi.lib().spl_eigsh_free(None)


def test_an_inner_solve_that_fails_is_reason_4(gpu, pkg):
    S = EK.matrix("grid")
    H, Hs = handle_of(pkg, S), handle_of(pkg, EK.shifted(S, 0.0))
    solver = pkg.KrylovSolver(Hs, "cg", None)
    E = Raw(pkg, gpu, H, 12)
    try:
        assert E.set_inverse(solver, 0.0, max_iter=1) == OK
        got = E.solve(start_of(S), 3, "LM")
        assert got.result == [4, 0, 0, 0, 1, 0] and got.untouched
        assert same_outcome(got, EK.inverse_reference(0.0, None, 3, 12, max_iter=1))
    finally:
        E.free()
        solver.free()


def test_refusals_in_the_header_s_order(gpu, pkg):
    lib = pkg._ffi.lib()
    S = EK.matrix("small")
    H = handle_of(pkg, S)
    e = C.c_void_p()
    # create
    assert lib.spl_eigsh_create(None, 0, None) == HANDLE
    assert lib.spl_eigsh_create(H.handle, 0, None) == MISSING
    e.value = 1
    rect = handle_of(pkg, sp.csr_matrix(np.ones((3, 4))))
    assert lib.spl_eigsh_create(rect.handle, 1, C.byref(e)) == MISSING and not e.value
    assert lib.spl_eigsh_create(rect.handle, 129, C.byref(e)) == MISSING
    assert lib.spl_eigsh_create(rect.handle, 4, C.byref(e)) == MISMATCH
    unsym = handle_of(pkg, sp.csr_matrix(np.triu(np.ones((4, 4)))))
    assert lib.spl_eigsh_create(unsym.handle, 4, C.byref(e)) == MATRIX and not e.value
    block = pkg.DeviceMatrix.synthetic("poisson2d", 4, row0=4, row1=12)  # rows 4 ... 11 of 16: square, but not whole
    assert lib.spl_eigsh_create(block.handle, 4, C.byref(e)) == MATRIX and not e.value
    skew = handle_of(pkg, sp.csr_matrix(np.array([[1.0, 1j], [1j, 2.0]])))
    assert lib.spl_eigsh_create(skew.handle, 2, C.byref(e)) == MATRIX
    # set_inverse
    E = Raw(pkg, gpu, H, 4)
    assert E.status == OK
    solver = pkg.KrylovSolver(H, "cg", None)
    other = pkg.KrylovSolver(handle_of(pkg, EK.matrix("ramp")), "cg", None)
    cplx = pkg.KrylovSolver(handle_of(pkg, sp.csr_matrix(S.astype(np.complex128))), "cg", None)
    try:
        assert lib.spl_eigsh_set_inverse(None, solver.handle, 0.0, 1e-12, 0.0, 10) == HANDLE
        assert lib.spl_eigsh_set_inverse(solver.handle, solver.handle, 0.0, 1e-12, 0.0, 10) == HANDLE
        assert lib.spl_eigsh_set_inverse(E.e, E.e, 0.0, -1.0, 0.0, -1) == HANDLE
        assert lib.spl_eigsh_set_inverse(E.e, other.handle, 0.0, -1.0, 0.0, -1) == MISMATCH
        assert lib.spl_eigsh_set_inverse(E.e, cplx.handle, 0.0, -1.0, 0.0, -1) == MISMATCH
        assert lib.spl_eigsh_set_inverse(E.e, solver.handle, 0.0, -1.0, 0.0, -1) == NONPOSITIVE
        for bad in ((0.0, -1.0, 0.0), (0.0, 0.0, float("nan")), (float("inf"), 1e-12, 0.0)):
            assert lib.spl_eigsh_set_inverse(E.e, solver.handle, bad[0], bad[1], bad[2], 10) == MISSING
        assert E.info()[2] == 0
        assert lib.spl_eigsh_set_inverse(E.e, None, float("nan"), -1.0, -1.0, -1) == OK  # K == NULL: nothing else is read
        # solve
        v0 = dev(gpu, start_of(S))
        X = gpu.zeros(3 * 8, dtype=gpu.float64, device="cuda")
        values, residuals, result = np.zeros(3), np.zeros(3), np.zeros(6, dtype=np.int64)
        history = np.zeros(4)

        def call(E_=E.e, nev=2, which=0, tol=1e-10, atol=0.0, restarts=3, v=v0.data_ptr(), val=values, x=X.data_ptr(),
                 ldx=8, res=residuals, out=result, hist=history):
            return lib.spl_eigsh_solve_dev(E_, nev, which, tol, atol, restarts, v, None if val is None else p_f64(val), x,
                                           ldx, None if res is None else p_f64(res), None if out is None else p_i64(out),
                                           None if hist is None else p_f64(hist), None)

        assert call(E_=None, val=None, restarts=0) == HANDLE
        assert call(E_=solver.handle, val=None) == HANDLE
        for name in ("val", "res", "out"):
            assert call(restarts=0, nev=0, **{name: None}) == MISSING
        assert call(restarts=0, nev=0) == NONPOSITIVE
        for bad in (dict(nev=0), dict(nev=4), dict(which=-1), dict(which=3), dict(tol=-1.0), dict(tol=float("nan")),
                    dict(atol=-1.0)):
            assert call(restarts=2 ** 31, **bad) == MISSING, bad
        assert call(restarts=2 ** 31, v=None) == OVERFLOW
        for bad in (dict(v=None), dict(x=None), dict(ldx=7)):
            assert call(**bad) == MISSING, bad
        assert call(hist=None) == OK and result[3] == 2
        big = Raw(pkg, gpu, H, 9)  # ncv > n
        assert big.status == OK and lib.spl_eigsh_solve_dev(big.e, 2, 0, 1e-10, 0.0, 3, v0.data_ptr(), p_f64(values),
                                                            X.data_ptr(), 8, p_f64(residuals), p_i64(result), None,
                                                            None) == MISSING
        big.free()
        assert lib.spl_eigsh_info(None, p_i64(result)) == HANDLE and lib.spl_eigsh_info(E.e, None) == MISSING
    finally:
        E.free()
        for k in (solver, other, cplx):
            k.free()


# ---- 4. the Python layer --------------------------------------------------------------------------------------------------------
def test_python_layer_gives_the_bits_of_the_raw_calls(gpu, pkg):
    S = EK.matrix("ramp")
    want = EK.reference("ramp", "LA", 3, 20, 1e-10, 200)
    H = handle_of(pkg, S)
    # the default ncv of nev = 3 is min(n, max(7, 20)) = 20, the default start default_rng(0).standard_normal
    values, X, res = H.eigsh(3, "LA", max_restarts=200)
    assert K.bits_equal(values, want.values) and K.bits_equal(X, want.vectors) and X.shape == (300, 3)
    assert K.bits_equal(res["residuals"], want.residuals) and K.bits_equal(res["history"], want.history)
    assert [res[k] for k in pkg.EigenSolver.RESULT_KEYS] == want.result and res["converged"] and res["reason_name"] == "converged"
    E = pkg.EigenSolver(H, 20)
    try:
        v0 = dev(gpu, start_of(S))
        values, X, res = E.solve(3, "LA", max_restarts=200, v0=v0)
        assert K.bits_equal(values, want.values) and K.bits_equal(X.cpu().numpy(), want.vectors)
        inf = E.info()
        assert inf["n"] == 300 and inf["ncv"] == 20 and not inf["complex"] and not inf["inverse"] and inf["solves"] == 1
    finally:
        E.free()
    host = pkg.Matrix(300, 300, sp.csc_matrix(S).indptr, sp.csc_matrix(S).indices, sp.csc_matrix(S).data)
    values, X, res = pkg.eigsh(host, 3, "LA", max_restarts=200)
    assert K.bits_equal(values, want.values) and K.bits_equal(X, want.vectors)
    # complex, and the inverse mode: `lin` makes A - sigma I and CG with Jacobi inverts it
    Z = EK.matrix("hermitian")
    zwant = EK.reference("hermitian", "LA", 3, 16, 1e-10, 200)
    values, X, res = handle_of(pkg, Z).eigsh(3, "LA", ncv=16, max_restarts=200)
    assert K.bits_equal(values, zwant.values) and K.bits_equal(X, zwant.vectors) and X.dtype == np.complex128
    G = handle_of(pkg, EK.matrix("grid"))
    iwant = EK.inverse_reference(5.0, "jacobi", 3, 12)
    values, X, res = G.eigsh(3, "LM", ncv=12, sigma=5.0, M="jacobi", max_restarts=200, inner_maxiter=EK.INNER_MAXITER)
    assert K.bits_equal(values, iwant.values) and K.bits_equal(X, iwant.vectors)
    assert [res[k] for k in pkg.EigenSolver.RESULT_KEYS] == iwant.result
    # the rotation through the layer
    V, Y, rotated = rotation_case(257, 3, 2, False)
    dV, dY = device_columns(gpu, V, 260), device_columns(gpu, Y, 3)
    pkg.sparse.vector_rotate_dev(257, 3, 2, dV.data_ptr(), 260, dY.data_ptr(), 3)
    gpu.cuda.synchronize()
    assert K.bits_equal(host_columns(dV, 257, 2, 260), rotated)
    with pytest.raises(ValueError):
        pkg.EigenSolver(H, 1)
    with pytest.raises(ValueError):
        H.eigsh(3, "XX")
