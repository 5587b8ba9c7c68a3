"""Restarted GMRES on device handles and its fused multi-vector inner product (csrc/gmres.hip), real and complex.  The
yardstick is the restatement of tests/gmres_cases.py (checked on its own in tests/test_gmres_cpu.py); the device's inner
products, iterates, counts, residual histories and residuals must equal it BIT FOR BIT, whatever the grid, the check
interval and the schedule of the preconditioner's solves are.  All comparisons are by view(uint64)."""
import ctypes as C
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as AK
import gmres_cases as GK
import krylov_cases as K

pytestmark = pytest.mark.gpu

HUGE = str(2 ** 30)
KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS", "SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH")
BOTH = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
COLUMNS = (1, 2, 3, 4, 5, 8, 33, 128)  # every remainder of the batch widths 2, 4 and 8


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def handle_of(pkg, S):
    """a whole device handle with the entries of the scipy matrix S (explicit zeros included), real or complex"""
    if S.shape[0] == 0:
        return pkg.DeviceMatrix.ident(0)
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


def pkg_p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def same_scalars(got, want):
    return K.bits_equal(np.atleast_1d(np.asarray(got)), np.atleast_1d(np.asarray(want)))


# ---- 1. k inner products in one pass -------------------------------------------------------------------------------------
def dots_inputs(n, cplx, k):
    """k columns and w of dot_inputs data: column 0 is w's own cancelling partner"""
    cols = []
    w = None
    for i in range(k):
        a, b = K.dot_inputs(n, cplx, seed=1 + i)
        cols.append(a)
        if i == 0:
            w = b
    return cols, w


def device_block(torch, cols, n, ldv, cplx):
    """the columns one after the other, ldv entries apart, the gaps filled with NaN (nothing may read them)"""
    dtype = np.complex128 if cplx else np.float64
    V = np.full(max(len(cols) * ldv, 1), np.nan, dtype=dtype)
    for i, c in enumerate(cols):
        V[i * ldv:i * ldv + n] = c
    return dev(torch, V)


def raw_dots(pkg, torch, n, k, dV, ldv, dw, cplx, stream="current"):
    out = torch.full((k,), 7.0, dtype=dw.dtype, device="cuda")
    s = torch.cuda.current_stream().cuda_stream if stream == "current" else stream
    st = pkg._ffi.lib().spl_vector_dots_dev(n, 2 if cplx else 1, k, dV.data_ptr() if n else None, ldv,
                                            dw.data_ptr() if n else None, out.data_ptr(), s)
    assert st == 0, st
    torch.cuda.synchronize()
    return out.cpu().numpy()


def raw_dot(pkg, torch, n, da_ptr, db_ptr, dtype, cplx):
    out = torch.full((1,), 7.0, dtype=dtype, device="cuda")
    st = pkg._ffi.lib().spl_vector_dot_dev(n, 2 if cplx else 1, da_ptr, db_ptr, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


@BOTH
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4095, 4096, 4097, 8281, 3 * 4096 + 5])
def test_dots_are_the_single_inner_products(gpu, pkg, monkeypatch, n, cplx):
    kmax = max(COLUMNS)
    cols, w = dots_inputs(n, cplx, kmax)
    want = np.array([K.dot(c, w) for c in cols])
    dw = dev(gpu, w) if n else gpu.zeros(1, dtype=gpu.complex128 if cplx else gpu.float64, device="cuda")
    step = 16 if cplx else 8
    for ldv in (n, n + 3):
        dV = device_block(gpu, cols, n, ldv, cplx)
        if n:  # the parent's only way: one call per column
            single = np.array([raw_dot(pkg, gpu, n, dV.data_ptr() + i * ldv * step, dw.data_ptr(), dw.dtype, cplx)
                               for i in range(kmax)])
            assert same_scalars(single, want)
        for grid in ("1", "2", None):
            if grid is None:
                monkeypatch.delenv("SPL_KRYLOV_GRID", raising=False)
            else:
                monkeypatch.setenv("SPL_KRYLOV_GRID", grid)
            for k in COLUMNS:
                got = raw_dots(pkg, gpu, n, k, dV, ldv, dw, cplx)
                assert same_scalars(got, want[:k]), (n, ldv, grid, k, int(np.argmax(got != want[:k])))
    if n == 0:
        assert not np.signbit(want.real).any() and not np.signbit(got.real).any()  # +0.0


def test_dots_batch_width_does_not_show(gpu, pkg, monkeypatch):
    n, k = 8281, 33
    for cplx in (False, True):
        cols, w = dots_inputs(n, cplx, k)
        want = np.array([K.dot(c, w) for c in cols])
        dV, dw = device_block(gpu, cols, n, n, cplx), dev(gpu, w)
        for width in ("2", "4", "8"):
            monkeypatch.setenv("SPL_GMRES_DOTS_BATCH", width)
            assert same_scalars(raw_dots(pkg, gpu, n, k, dV, n, dw, cplx), want), width


def test_dots_three_levels(gpu, pkg):
    """4096^2 + 5 entries: 4097 chunks, whose partials are two chunks of the second level, whose partials the third
    level folds; the only length that reaches it"""
    n = 4096 * 4096 + 5
    rng = np.random.default_rng(93)
    w = rng.standard_normal(n)
    cols = [w * np.where((np.arange(n) // 5) % 2 == 0, 1.0, -1.0), rng.standard_normal(n)]
    want = np.array([K.dot(c, w) for c in cols])
    dV = gpu.empty(2 * n, dtype=gpu.float64, device="cuda")
    dV[:n].copy_(gpu.from_numpy(cols[0]))
    dV[n:].copy_(gpu.from_numpy(cols[1]))
    got = raw_dots(pkg, gpu, n, 2, dV, n, dev(gpu, w), False)
    assert same_scalars(got, want), (got, want)
    assert abs(want[0]) < 1e-3 * n  # it cancels


def test_dots_from_several_threads_on_one_stream_do_not_share_partials(gpu, pkg):
    """every call has its own block for the partials: four threads on the default stream, forty calls each"""
    cases = []
    for n, cplx, k in [(4096, False, 5), (8229, True, 3), (20005, False, 8), (12000, True, 33)]:
        cols, w = dots_inputs(n, cplx, k)
        cases.append((device_block(gpu, cols, n, n, cplx), dev(gpu, w), np.array([K.dot(c, w) for c in cols]), n, cplx, k))
    L = pkg._ffi.lib()
    wrong, errors = [], []
    start = threading.Barrier(len(cases))

    def work(slot):
        try:
            gpu.cuda.set_device(0)
            dV, dw, want, n, cplx, k = cases[slot]
            outs = gpu.zeros(40 * k, dtype=dw.dtype, device="cuda")
            step = (16 if cplx else 8) * k
            start.wait()
            for c in range(40):
                st = L.spl_vector_dots_dev(n, 2 if cplx else 1, k, dV.data_ptr(), n, dw.data_ptr(),
                                           outs.data_ptr() + c * step, None)
                assert st == 0, st
            gpu.cuda.synchronize()
            got = outs.cpu().numpy().reshape(40, k)
            wrong.extend((slot, c) for c in range(40) if not same_scalars(got[c], want))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(cases))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not wrong, wrong


def test_vector_dots_dev_of_the_python_layer(gpu, pkg):
    for cplx in (False, True):
        cols, w = dots_inputs(8229, cplx, 4)
        dV, dw = device_block(gpu, cols, 8229, 8232, cplx), dev(gpu, w)
        out = gpu.zeros(4, dtype=dw.dtype, device="cuda")
        pkg.vector_dots_dev(8229, 4, dV.data_ptr(), 8232, dw.data_ptr(), out.data_ptr(), is_complex=cplx,
                            stream=gpu.cuda.current_stream().cuda_stream)
        gpu.cuda.synchronize()
        assert same_scalars(out.cpu().numpy(), np.array([K.dot(c, w) for c in cols]))


# ---- 2. the solver ---------------------------------------------------------------------------------------------------------
class Raw(object):
    """spl_gmres_* through ctypes, nothing of the Python layer in between"""

    def __init__(self, pkg, torch, H, restart):
        self.pkg, self.torch, self.L = pkg, torch, pkg._ffi.lib()
        self.H = H
        self.cplx = H.is_complex
        self.n = H.info()["nrows_global"]
        self.g = C.c_void_p()
        assert self.L.spl_gmres_create(H.handle, restart, C.byref(self.g)) == 0
        self.keep = ()

    def set(self, T1=None, mid=None, T2=None):
        self.keep = (T1, mid, T2)
        return self.L.spl_gmres_set_preconditioner(self.g, T1.handle if T1 is not None else None,
                                                   mid.data_ptr() if mid is not None else None,
                                                   T2.handle if T2 is not None else None)

    def solve(self, b, x0=None, rtol=GK.RTOL, atol=0.0, max_iter=2000, check_every=0, history=True):
        torch = self.torch
        db = dev(torch, b)
        dtype = torch.complex128 if self.cplx else torch.float64
        dx = dev(torch, x0) if x0 is not None else torch.full((max(self.n, 1),), 7.0, dtype=dtype, device="cuda")
        result = (C.c_int64 * 6)(*([-1] * 6))
        residual = np.full(2, -1.0)
        hist = np.full(max_iter + 1, -1.0)
        st = self.L.spl_gmres_solve_dev(self.g, db.data_ptr(), dx.data_ptr(), 1 if x0 is not None else 0, rtol, atol,
                                        max_iter, check_every, result, pkg_p(hist) if history else None, pkg_p(residual),
                                        torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
        return dx.cpu().numpy()[:self.n], list(result), hist[:result[0] + 1], residual

    def info(self):
        out = (C.c_int64 * 8)()
        assert self.L.spl_gmres_info(self.g, out) == 0
        return list(out)

    def free(self):
        self.L.spl_gmres_free(C.byref(self.g))


def device_parts(pkg, torch, H, S, kind):
    """(T1, mid, T2, owner) on the device for the preconditioner `kind` of the scipy matrix S behind the handle H"""
    if kind is None:
        return None, None, None, None
    if kind == "jacobi":
        return None, dev(torch, K.reciprocal_diagonal(S)), None, None
    if kind == "sgs":
        return H.triangular("lower"), dev(torch, sp.csr_matrix(S).diagonal()), H.triangular("upper"), None
    I = H.ilu0()
    return I.lower, None, I.upper, I


def assert_outcome(got, want, what=""):
    x, result, hist, residual = got
    assert (result[0], result[1], result[2]) == (want.iterations, want.reason, want.cycles), \
        (what, result, want.iterations, want.reason, want.cycles)
    assert K.bits_equal(hist, want.history), (what, "history", int(np.argmax(hist != want.history)))
    assert K.bits_equal(residual, want.residual), (what, "residual", residual, want.residual)
    assert K.bits_equal(x, want.x), (what, "x", float(np.max(np.abs(x - want.x))))
    assert result[3] >= want.spmvs and result[4] >= want.applications and result[5] == 0, (what, result)


@pytest.mark.parametrize("name,kind,restart,max_iter", GK.CASES, ids=lambda v: str(v))
def test_solver_bit_for_bit(gpu, pkg, name, kind, restart, max_iter):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, restart)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = GK.reference(name, kind, restart, max_iter)
    assert want.reason == (1 if max_iter < 2000 else 0)
    if max_iter < 2000:  # reason 1 at a cycle boundary (60 = 2 * 30) and in mid cycle (45)
        assert want.iterations == max_iter and (max_iter % restart == 0) == (name == "poisson")
    got = R.solve(K.rhs(name), max_iter=max_iter)
    assert_outcome(got, want, (name, kind, restart))
    inf = R.info()
    flags = (1 if np.iscomplexobj(S.data) else 0) | (2 if T1 is not None else 0) | (4 if mid is not None else 0) | \
        (8 if T2 is not None else 0)
    vector_bytes = S.shape[0] * (16 if flags & 1 else 8)
    assert inf[:3] == [S.shape[0], restart, flags] and inf[4] == 1 and inf[5] == want.iterations and inf[7] == 0
    assert inf[3] >= (restart + 3) * vector_bytes and inf[3] < (restart + 4) * vector_bytes + (1 << 20)
    assert inf[6] >= 9 * want.iterations  # SpMV, two passes of three launches, the scalar step, the division
    # a look after every cycle: whole cycles are issued, and the start after the last one
    assert got[1][3] == restart * want.cycles + want.cycles
    assert (got[1][4] > 0) == (kind is not None)
    R.free()
    if owner is not None:
        owner.free()


@pytest.mark.parametrize("name,kind,restart", [("shifted", "jacobi", 1), ("unsym", "ilu0", 5)])
def test_a_nonzero_start(gpu, pkg, name, kind, restart):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, restart)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = GK.reference(name, kind, restart, start=True)
    assert want.reason == 0 and not K.bits_equal(want.history[:1], GK.reference(name, kind, restart).history[:1])
    assert_outcome(R.solve(K.rhs(name), x0=K.start_vector(name)), want)
    R.free()


def test_amg_cycle_as_the_preconditioner(gpu, pkg):
    name, restart = "poisson", 20
    S, b = K.matrix(name), np.array(K.rhs(name))
    H = handle_of(pkg, S)
    M = H.amg()
    levels = [AK.Level(scipy_of(g["A"]), g["w"].cpu().numpy(), None if g["P"] is None else scipy_of(g["P"]),
                       None if g["R"] is None else scipy_of(g["R"])) for g in (M.level(l) for l in range(M.levels))]
    want = GK.gmres(K._operator(name), b, AK.Cycle(levels, 1, 4), None, restart, GK.RTOL, 0.0, 2000)
    assert want.reason == 0
    R = Raw(pkg, gpu, H, restart)
    assert R.L.spl_gmres_set_preconditioner_amg(R.g, M.handle) == 0
    assert R.info()[2] == 16
    assert_outcome(R.solve(b), want, "amg")
    plain = GK.reference(name, None, 30, 60)
    print("poisson, GMRES(20) with the cycle: %d iterations in %d cycles (without: more than %d)"
          % (want.iterations, want.cycles, plain.iterations))
    assert R.L.spl_gmres_set_preconditioner_amg(R.g, None) == 0 and R.info()[2] == 0
    R.free()
    M.free()


# ---- 3. the check interval, the grid and the schedules do not show -----------------------------------------------------------
INVARIANT = [("poisson", "ilu0", 30), ("unsymz", "jacobi", 5)]  # one real, one complex


@pytest.mark.parametrize("name,kind,restart", INVARIANT)
def test_check_every_and_the_grid_do_not_show(gpu, pkg, monkeypatch, name, kind, restart):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, restart)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = GK.reference(name, kind, restart)
    issued = {}
    for every in (1, 3):
        got = R.solve(K.rhs(name), check_every=every)
        assert_outcome(got, want, every)
        issued[every] = got[1][3]
    assert issued[1] == (restart + 1) * want.cycles
    assert issued[3] == (restart + 1) * 3 * -(-want.cycles // 3) and issued[3] >= issued[1]
    for grid in ("1", "2"):
        monkeypatch.setenv("SPL_KRYLOV_GRID", grid)
        assert_outcome(R.solve(K.rhs(name)), want, grid)
    R.free()


@pytest.mark.parametrize("name,kind,restart", [("poisson", "ilu0", 30), ("unsymz", "sgs", 30)])
def test_schedule_of_the_solves_does_not_show(gpu, pkg, monkeypatch, name, kind, restart):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    want = GK.reference(name, kind, restart)
    launches = set()
    for small in ("1", HUGE):
        monkeypatch.setenv("SPL_TRSV_SMALL_ROWS", small)  # read by the analysis of the triangular solvers
        R = Raw(pkg, gpu, H, restart)
        T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
        assert R.set(T1, mid, T2) == 0
        assert_outcome(R.solve(K.rhs(name)), want, small)
        launches.add(R.info()[6])
        R.free()
    assert len(launches) == 2  # the knob was read: the launches differ


# ---- 4. endings --------------------------------------------------------------------------------------------------------------
def test_twice_the_identity_closes_on_eta(gpu, pkg):
    n = 5000
    b = np.zeros(n)
    b[:4096] = 1.0  # |b| = 64: v_0 and <v_0, A v_0> are exact, so w vanishes exactly and eta == 0 closes the cycle
    S = sp.csr_matrix(2.0 * sp.identity(n))
    want = GK.gmres(S, b)
    assert (want.iterations, want.reason, want.cycles) == (1, 0, 1) and want.history[1] == 0.0
    R = Raw(pkg, gpu, handle_of(pkg, S), 30)
    assert_outcome(R.solve(b), want, "2 I")
    R.free()


def test_breakdown_and_what_is_not_finite(gpu, pkg):
    n = 5
    start = np.arange(1.0, 6.0)
    zeros = sp.csr_matrix((np.zeros(n), np.arange(n), np.arange(n + 1)), shape=(n, n))  # stored zeros
    R = Raw(pkg, gpu, handle_of(pkg, zeros), 30)
    want = GK.gmres(zeros, np.ones(n), x0=start)
    assert (want.iterations, want.reason) == (0, 2)
    got = R.solve(np.ones(n), x0=start)
    assert_outcome(got, want, "stored zeros")
    assert np.array_equal(got[0], start)
    R.free()
    bad = np.eye(n)
    bad[1, 2] = np.inf
    bad = sp.csr_matrix(bad)
    R = Raw(pkg, gpu, handle_of(pkg, bad), 30)
    want = GK.gmres(bad, np.ones(n))
    got = R.solve(np.ones(n))
    assert (want.iterations, want.reason) == (0, 3) and got[1][:3] == [0, 3, 1]
    assert K.bits_equal(got[2], want.history) and not got[0].any()
    R.free()
    two = sp.csr_matrix(2.0 * np.eye(n))
    R = Raw(pkg, gpu, handle_of(pkg, two), 30)
    nan = np.ones(n)
    nan[3] = np.nan
    got = R.solve(nan)
    assert got[1][:3] == [0, 3, 0] and np.isnan(got[2][0]) and got[1][3] == 0  # at the start: nothing was issued
    # b = 0: x = 0 after 0 iterations, converged
    x, result, hist, residual = R.solve(np.zeros(n))
    assert result[:3] == [0, 0, 0] and not x.any() and hist.tolist() == [0.0] and residual.tolist() == [0.0, 0.0]
    # max_iter 0: the start alone
    x, result, hist, residual = R.solve(np.ones(n), max_iter=0)
    assert result[:3] == [0, 1, 0] and not x.any() and result[3] == 0
    R.free()


def test_restart_longer_than_the_system(gpu, pkg):
    small = sp.csr_matrix(np.array([[4.0, 1.0, 0.0], [2.0, 5.0, 1.0], [0.0, -1.0, 3.0]]))
    b = np.array([1.0, 2.0, 3.0])
    want = GK.gmres(small, b, restart=30)
    assert want.reason == 0 and want.iterations <= 4
    R = Raw(pkg, gpu, handle_of(pkg, small), 30)
    assert_outcome(R.solve(b), want, "n = 3")
    R.free()


def test_an_empty_system(gpu, pkg):
    H = pkg.DeviceMatrix.ident(0)
    R = Raw(pkg, gpu, H, 30)
    result = (C.c_int64 * 6)(*([-1] * 6))
    residual = np.full(2, -1.0)
    hist = np.full(3, -1.0)
    assert R.L.spl_gmres_solve_dev(R.g, None, None, 0, 1e-8, 0.0, 2, 0, result, pkg_p(hist), pkg_p(residual), None) == 0
    assert list(result) == [0] * 6 and hist[0] == 0.0 and residual.tolist() == [0.0, 0.0]
    assert R.L.spl_gmres_solve(R.g, None, None, 0, 1e-8, 0.0, 2, result, None, pkg_p(residual)) == 0
    assert R.info()[0] == 0
    R.free()


# ---- 5. the object, the host-vector call and the Python layer ----------------------------------------------------------------
def test_solves_in_a_row_info_and_free(gpu, pkg):
    name, kind, restart = "unsymz", "jacobi", 5
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, restart)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = GK.reference(name, kind, restart)
    first = R.solve(K.rhs(name))
    second = R.solve(K.rhs(name))
    assert_outcome(first, want, "first")
    assert_outcome(second, want, "second")
    inf = R.info()
    assert inf[4] == 2 and inf[5] == want.iterations and inf[6] > 0
    # the host-vector call gives the bits of the device call
    b = np.array(K.rhs(name))
    x = np.zeros_like(b)
    result = (C.c_int64 * 6)(*([-1] * 6))
    residual = np.full(2, -1.0)
    hist = np.full(2001, -1.0)
    assert R.L.spl_gmres_solve(R.g, pkg_p(b.view(np.float64)), pkg_p(x.view(np.float64)), 0, GK.RTOL, 0.0, 2000, result,
                               pkg_p(hist), pkg_p(residual)) == 0
    assert_outcome((x, list(result), hist[:result[0] + 1], residual), want, "host vectors")
    assert R.info()[4] == 3
    R.free()
    R.free()
    assert not R.g.value


def test_parts_of_another_size_or_kind_are_refused(gpu, pkg):
    F = pkg._ffi
    H = handle_of(pkg, K.matrix("unsym"))
    R = Raw(pkg, gpu, H, 5)
    small = handle_of(pkg, sp.identity(7, format="csr")).triangular("lower")
    cplx = handle_of(pkg, K.matrix("unsymz")).triangular("lower")
    good = H.triangular("upper")
    assert R.set(small, None, None) == F.SPL_ERROR_dimension_mismatch
    assert R.set(cplx, None, None) == F.SPL_ERROR_dimension_mismatch
    assert R.L.spl_gmres_set_preconditioner(R.g, H.handle, None, None) == F.SPL_ERROR_invalid_handle  # a matrix is no solver
    assert R.info()[2] == 0  # nothing was set
    assert R.set(None, None, good) == 0 and R.info()[2] == 8
    assert R.set() == 0 and R.info()[2] == 0
    R.free()


def host_matrix(pkg, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    return pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)


@pytest.mark.parametrize("name", ["unsym", "shifted"])
def test_python_layer_gives_the_bits_of_the_raw_calls(gpu, pkg, name):
    S, b = K.matrix(name), np.array(K.rhs(name))
    H = handle_of(pkg, S)
    restart = 30

    def outcome(x, res):
        return (x, [res["iterations"], res["reason"], res["cycles"], res["spmvs"], res["preconditioner_applications"], 0],
                res["history"], np.array([res["residual"], res["estimate"]]))

    for kind in (None, "ilu0", "jacobi"):
        M = H.ilu0() if kind == "ilu0" else kind
        solver = H.gmres(restart, M)
        if kind == "jacobi":  # the layer makes 1 / diag with torch: the yardstick is given what the device was given
            want = GK.gmres(S, b, K.preconditioner(S, "jacobi", solver.parts[1].cpu().numpy()), None, restart, GK.RTOL, 0.0,
                            2000)
        else:
            want = GK.reference(name, kind, restart)
        x, res = solver.solve(b, maxiter=2000)
        assert isinstance(x, np.ndarray) and res["converged"] and res["reason_name"] == "converged"
        assert_outcome(outcome(x, res), want, ("solve", kind))
        x, res = solver.solve(b, maxiter=2000, check_every=2)
        assert_outcome(outcome(x, res), want, ("solve, check_every", kind))
        tx, res = solver.solve(dev(gpu, b), maxiter=2000)
        assert tx.is_cuda
        assert_outcome(outcome(tx.cpu().numpy(), res), want, ("tensor", kind))
        inf = solver.info()
        assert inf["n"] == S.shape[0] and inf["restart"] == restart and inf["solves"] == 3
        assert inf["complex"] == np.iscomplexobj(S.data) and inf["iterations"] == want.iterations
        assert (inf["T1"], inf["mid"], inf["T2"]) == {None: (False, False, False), "ilu0": (True, False, True),
                                                      "jacobi": (False, True, False)}[kind]
        solver.free()
        solver.free()
    host = host_matrix(pkg, S)
    x, res = pkg.gmres(host, b, M="sgs", restart=restart, maxiter=2000)
    assert_outcome(outcome(x, res), GK.reference(name, "sgs", restart), "sparse.gmres")
    # the true residual norm of the x that is returned; the margin: numpy's norm of b is not the fold's
    assert res["residual"] <= GK.RTOL * np.linalg.norm(b) * (1 + 1e-12)
    started = GK.reference(name, None, restart, start=True)
    x, res = pkg.gmres(host, b, x0=np.array(K.start_vector(name)), restart=restart, maxiter=2000)
    assert_outcome(outcome(x, res), started, "sparse.gmres with a start")
    # the CG / BiCGSTAB layer is what it was
    xb, resb = pkg.bicgstab(host, b, M="sgs", maxiter=2000)
    ref = K.reference("bicgstab", name, "sgs")
    assert resb["iterations"] == ref.iterations and K.bits_equal(xb, ref.x) and sorted(resb) == sorted(
        ["iterations", "reason", "reason_name", "converged", "spmvs", "preconditioner_applications", "history"])
