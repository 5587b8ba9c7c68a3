"""Preconditioned CG and BiCGSTAB on device handles and their fixed-order inner product (csrc/krylov.hip), real and
complex.  The yardstick is the restatement of tests/krylov_cases.py (checked on its own in tests/test_krylov_cpu.py); the
device's inner products, iterates, iteration counts and residual histories must equal it BIT FOR BIT, whatever the grid,
the check interval and the schedule of the preconditioner's solves are.  All comparisons are by view(uint64)."""
import ctypes as C
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import krylov_cases as K

pytestmark = pytest.mark.gpu

HUGE = str(2 ** 30)
KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS", "SPL_KRYLOV_GRID")
BOTH = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
METHOD = {"cg": 0, "bicgstab": 1}


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def handle_of(pkg, S):
    """a whole device handle with the entries of the scipy matrix S, real or complex"""
    S = sp.csc_matrix(S)
    S.sort_indices()
    M = pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)
    return pkg.DeviceMatrix.from_csc_complex(M) if np.iscomplexobj(S.data) else pkg.DeviceMatrix.from_csc(M)


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the cached inputs are read-only


def raw_dot(pkg, torch, a, b):
    """spl_vector_dot_dev on two device tensors: a float or a complex"""
    cplx = a.dtype == torch.complex128
    out = torch.full((1,), 7.0, dtype=a.dtype, device="cuda")
    st = pkg._ffi.lib().spl_vector_dot_dev(int(a.shape[0]), 2 if cplx else 1, a.data_ptr(), b.data_ptr(), out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    v = out.cpu().numpy()[0]
    return complex(v) if cplx else float(v)


def same_scalar(got, want):
    got, want = np.atleast_1d(np.asarray(got)), np.atleast_1d(np.asarray(want))
    return K.bits_equal(got, want)


class Raw(object):
    """spl_krylov_* through ctypes, nothing of the Python layer in between"""

    def __init__(self, pkg, torch, H, method):
        self.pkg, self.torch, self.L = pkg, torch, pkg._ffi.lib()
        self.H = H
        self.cplx = H.is_complex
        self.n = H.info()["nrows_global"]
        self.k = C.c_void_p()
        assert self.L.spl_krylov_create(H.handle, METHOD[method], C.byref(self.k)) == 0
        self.keep = ()

    def set(self, T1=None, mid=None, T2=None):
        self.keep = (T1, mid, T2)
        return self.L.spl_krylov_set_preconditioner(self.k, T1.handle if T1 is not None else None,
                                                    mid.data_ptr() if mid is not None else None,
                                                    T2.handle if T2 is not None else None)

    def solve(self, b, x0=None, rtol=K.RTOL, atol=0.0, max_iter=2000, check_every=0, history=True):
        torch = self.torch
        db = dev(torch, b)
        dtype = torch.complex128 if self.cplx else torch.float64
        dx = dev(torch, x0) if x0 is not None else torch.full((max(self.n, 1),), 7.0, dtype=dtype, device="cuda")
        result = (C.c_int64 * 4)(-1, -1, -1, -1)
        hist = np.full(max_iter + 1, -1.0)
        st = self.L.spl_krylov_solve_dev(self.k, db.data_ptr(), dx.data_ptr(), 1 if x0 is not None else 0, rtol, atol,
                                         max_iter, check_every, result, pkg_p(hist) if history else None,
                                         torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
        return dx.cpu().numpy()[:self.n], list(result), hist[:result[0] + 1]

    def info(self):
        out = (C.c_int64 * 8)()
        assert self.L.spl_krylov_info(self.k, out) == 0
        return list(out)

    def free(self):
        self.L.spl_krylov_free(C.byref(self.k))


def pkg_p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


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
    x, result, hist = got
    assert (result[0], result[1]) == (want.iterations, want.reason), (what, result, want.iterations, want.reason)
    assert K.bits_equal(hist, want.history), (what, "history", int(np.argmax(hist != want.history)))
    assert K.bits_equal(x, want.x), (what, "x", float(np.max(np.abs(x - want.x))))


# ---- 1. the fold -------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4095, 4096, 4097, 8229, 20005])
def test_fold_up_to_20005_entries(gpu, pkg, n, cplx):
    a, b = K.dot_inputs(n, cplx)
    got = raw_dot(pkg, gpu, dev(gpu, a), dev(gpu, b))
    assert same_scalar(got, K.dot(a, b)), (n, got, K.dot(a, b))
    if n == 0:
        assert np.signbit(np.real(got)) == False  # noqa: E712  (+0.0)


@BOTH
def test_fold_three_levels(gpu, pkg, cplx):
    """4096^2 + 5 entries: 4097 chunks, whose partials are two chunks of the second level, whose partials the third
    level folds; the only length that reaches it"""
    n = 4096 * 4096 + 5
    rng = np.random.default_rng(91 + cplx)
    a = rng.standard_normal(n)
    if cplx:
        a = a + 1j * rng.standard_normal(n)
    b = a * np.where((np.arange(n) // 5) % 2 == 0, 1.0, -1.0)  # cancelling runs
    got = raw_dot(pkg, gpu, dev(gpu, a), dev(gpu, b))
    want = K.dot(a, b)
    assert same_scalar(got, want), (got, want)
    assert abs(want) < 1e-3 * n  # it cancels


def test_calls_from_several_threads_on_one_stream_do_not_share_partials(gpu, pkg):
    """every call has its own block for the partials: four threads on the default stream, lengths of one, three and
    five chunks, real and complex, forty calls each, every value the restatement's"""
    cases = []
    for i, (n, cplx) in enumerate([(4096, False), (8229, True), (20005, False), (12000, True)]):
        a, b = K.dot_inputs(n, cplx, seed=10 + i)
        cases.append((dev(gpu, a), dev(gpu, b), K.dot(a, b), cplx))
    L = pkg._ffi.lib()
    wrong, errors = [], []
    start = threading.Barrier(len(cases))

    def work(slot):
        try:
            gpu.cuda.set_device(0)
            da, db, want, cplx = cases[slot]
            outs = gpu.zeros(40, dtype=da.dtype, device="cuda")
            step = 16 if cplx else 8
            start.wait()
            for k in range(40):
                st = L.spl_vector_dot_dev(int(da.shape[0]), 2 if cplx else 1, da.data_ptr(), db.data_ptr(),
                                          outs.data_ptr() + k * step, None)
                assert st == 0, st
            gpu.cuda.synchronize()
            got = outs.cpu().numpy()
            wrong.extend((slot, k) for k in range(40) if not same_scalar(got[k], want))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(cases))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not wrong, wrong


@BOTH
def test_the_grid_does_not_show_in_the_bits(gpu, pkg, monkeypatch, cplx):
    a, b = K.dot_inputs(20005, cplx, seed=2)
    da, db = dev(gpu, a), dev(gpu, b)
    want = K.dot(a, b)
    for grid in ("1", "2", "3", "4", "65535"):
        monkeypatch.setenv("SPL_KRYLOV_GRID", grid)  # one workgroup takes all five chunks, ..., one each
        assert same_scalar(raw_dot(pkg, gpu, da, db), want), grid
    name, method = ("hermitian", "cg") if cplx else ("poisson", "bicgstab")
    R = Raw(pkg, gpu, handle_of(pkg, K.matrix(name)), method)
    for grid in ("1", "2"):
        monkeypatch.setenv("SPL_KRYLOV_GRID", grid)
        assert_outcome(R.solve(K.rhs(name)), K.reference(method, name, None), grid)
    R.free()


# ---- 2. the drivers: x, the iteration count and the whole history ------------------------------------------------------
@pytest.mark.parametrize("kind", K.PRECONDITIONERS, ids=lambda k: str(k))
@pytest.mark.parametrize("method,name", K.CASES)
def test_drivers_bit_for_bit(gpu, pkg, method, name, kind):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, method)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = K.reference(method, name, kind)
    got = R.solve(K.rhs(name))
    assert_outcome(got, want, (method, name, kind))
    inf = R.info()
    flags = (1 if np.iscomplexobj(S.data) else 0) | (2 if T1 is not None else 0) | (4 if mid is not None else 0) | \
        (8 if T2 is not None else 0)
    assert inf[:3] == [S.shape[0], METHOD[method], flags] and inf[3] > 0 and inf[4] == 1 and inf[5] == want.iterations
    # launches per iteration: without a preconditioner CG does not compute <r,z> = <r,r> again (6, not 8)
    own = {("cg", None): 6, ("cg", "jacobi"): 9, ("bicgstab", None): 13, ("bicgstab", "jacobi"): 15}
    if (method, kind) in own:
        assert inf[6] == own[(method, kind)]
    assert inf[6] >= (6 if method == "cg" else 13) and inf[7] == 0
    # issued work: one SpMV per CG iteration, two per BiCGSTAB iteration; the host stops at a check, never before
    per = 1 if method == "cg" else 2
    assert got[1][2] >= per * want.iterations - 1 and got[1][2] <= per * (want.iterations + 16)
    assert (got[1][3] > 0) == (kind is not None)
    R.free()
    if owner is not None:
        owner.free()


@pytest.mark.parametrize("method,name,kind", [("cg", "poisson", "ilu0"), ("cg", "hermitian", "jacobi"),
                                              ("bicgstab", "shifted", "sgs"), ("bicgstab", "unsym", None)])
def test_a_nonzero_start(gpu, pkg, method, name, kind):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, method)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = K.reference(method, name, kind, start=True)
    assert want.reason == 0 and not K.bits_equal(want.history[:1], K.reference(method, name, kind).history[:1])
    assert_outcome(R.solve(K.rhs(name), x0=K.start_vector(name)), want)
    R.free()


# ---- 3. the check interval and the schedules do not show ---------------------------------------------------------------
@pytest.mark.parametrize("method,name,kind", [("cg", "poisson", "ilu0"), ("bicgstab", "shifted", None)])
def test_check_every_does_not_show(gpu, pkg, method, name, kind):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, method)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = K.reference(method, name, kind)
    issued = {}
    for every in (1, 3, 64):
        got = R.solve(K.rhs(name), check_every=every)
        assert_outcome(got, want, every)
        issued[every] = got[1][2]
    print("SpMVs issued for %d iterations at check_every 1, 3, 64: %s" % (want.iterations, issued))
    per = 1 if method == "cg" else 2
    assert issued[1] == per * want.iterations  # a look after every iteration: nothing is issued for nothing
    assert issued[64] == per * 64 * -(-want.iterations // 64) and issued[64] > issued[1]
    R.free()


@pytest.mark.parametrize("method,name,kind", [("cg", "poisson", "ilu0"), ("bicgstab", "unsymz", "sgs")])
def test_schedule_of_the_solves_does_not_show(gpu, pkg, monkeypatch, method, name, kind):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    want = K.reference(method, name, kind)
    launches = set()
    for small in ("1", HUGE):
        monkeypatch.setenv("SPL_TRSV_SMALL_ROWS", small)  # read by the analysis of the triangular solvers
        R = Raw(pkg, gpu, H, method)
        T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
        assert R.set(T1, mid, T2) == 0
        assert_outcome(R.solve(K.rhs(name)), want, small)
        launches.add(R.info()[6])
        R.free()
    assert len(launches) == 2  # the knob was read: the launches per iteration differ


# ---- 4. endings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,name", [("cg", "poisson"), ("cg", "hermitian"), ("bicgstab", "poisson"),
                                         ("bicgstab", "shifted")])
def test_max_iter_three_is_the_third_iterate(gpu, pkg, method, name):
    R = Raw(pkg, gpu, handle_of(pkg, K.matrix(name)), method)
    want = K.reference(method, name, None, max_iter=3)
    assert (want.iterations, want.reason) == (3, 1)
    assert_outcome(R.solve(K.rhs(name), max_iter=3), want)
    zero = R.solve(K.rhs(name), max_iter=0)
    assert zero[1][:2] == [0, 1] and not zero[0].any() and K.bits_equal(zero[2], want.history[:1])
    R.free()


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_small_systems_and_breakdown(gpu, pkg, method):
    drive = K.DRIVERS[method]
    # A = -I: CG converges on it, which is allowed
    minus = sp.csr_matrix(-np.eye(5))
    b = np.arange(1.0, 6.0)
    R = Raw(pkg, gpu, handle_of(pkg, minus), method)
    want = drive(minus, b)
    assert want.reason == 0
    assert_outcome(R.solve(b), want, "-I")
    # b = 0: x = 0 after 0 iterations, converged
    x, result, hist = R.solve(np.zeros(5))
    assert result[:2] == [0, 0] and not x.any() and hist.tolist() == [0.0]
    # a NaN in b: reason 3 within one check interval
    bad = b.copy()
    bad[2] = np.nan
    x, result, hist = R.solve(bad, check_every=4)
    assert result[:2] == [0, 3] and result[2] <= 4 * (1 if method == "cg" else 2)
    R.free()
    # singular and inconsistent: breakdown or max_iter, never an error and never a hang
    S2 = sp.csr_matrix(np.array([[1.0, 1.0], [1.0, 1.0]]))
    R = Raw(pkg, gpu, handle_of(pkg, S2), method)
    want = drive(S2, np.array([1.0, 0.0]), max_iter=50)
    got = R.solve(np.array([1.0, 0.0]), max_iter=50)
    assert got[1][1] in (1, 2) and (got[1][0], got[1][1]) == (want.iterations, want.reason)
    assert K.bits_equal(got[2], want.history)
    R.free()
    # n = 1
    one = sp.csr_matrix(np.array([[2.0]]))
    R = Raw(pkg, gpu, handle_of(pkg, one), method)
    want = drive(one, np.array([3.0]))
    assert_outcome(R.solve(np.array([3.0])), want, "n = 1")
    assert want.x.tolist() == [1.5]
    R.free()


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_an_empty_system(gpu, pkg, method):
    H = pkg.DeviceMatrix.ident(0)
    R = Raw(pkg, gpu, H, method)
    result = (C.c_int64 * 4)(-1, -1, -1, -1)
    hist = np.full(3, -1.0)
    assert R.L.spl_krylov_solve_dev(R.k, None, None, 0, 1e-8, 0.0, 2, 0, result, pkg_p(hist), None) == 0
    assert list(result) == [0, 0, 0, 0] and hist[0] == 0.0
    assert R.L.spl_krylov_solve(R.k, None, None, 0, 1e-8, 0.0, 2, result, None) == 0
    assert R.info()[0] == 0
    R.free()


# ---- 5. quality, beyond bits -------------------------------------------------------------------------------------------
def test_ilu0_pcg_on_poisson3d(gpu, pkg):
    """poisson3d(30), rtol 1e-10: the true residual, computed on the host, and fewer iterations than without M; both
    shown for the restatement in tests/test_krylov_cpu.py"""
    S, b = K.matrix("poisson3d"), K.rhs("poisson3d")
    H = handle_of(pkg, S)
    I = H.ilu0()
    R = Raw(pkg, gpu, H, "cg")
    plain = R.solve(b, rtol=1e-10)
    assert R.set(I.lower, None, I.upper) == 0
    pre = R.solve(b, rtol=1e-10)
    assert plain[1][1] == 0 and pre[1][1] == 0
    true = K.true_relative_residual(S, pre[0], b)
    print("poisson3d(30): %d iterations with ILU(0), %d without; true relative residual %.3e" % (pre[1][0], plain[1][0], true))
    assert true <= 10 * 1e-10
    assert pre[1][0] < plain[1][0]
    assert_outcome(pre, K.reference("cg", "poisson3d", "ilu0", rtol=1e-10))
    R.free()
    I.free()


# ---- 6. the objects ----------------------------------------------------------------------------------------------------
def test_solves_in_a_row_and_from_two_threads(gpu, pkg):
    name, method, kind = "hermitian", "cg", "sgs"
    S = K.matrix(name)
    H = handle_of(pkg, S)
    R = Raw(pkg, gpu, H, method)
    T1, mid, T2, owner = device_parts(pkg, gpu, H, S, kind)
    assert R.set(T1, mid, T2) == 0
    want = K.reference(method, name, kind)
    other = K.reference(method, name, kind, start=True)
    assert_outcome(R.solve(K.rhs(name)), want, "first")
    assert_outcome(R.solve(K.rhs(name), x0=K.start_vector(name)), other, "second, another start")
    assert_outcome(R.solve(K.rhs(name)), want, "third")
    assert R.info()[4] == 3
    results, errors = {}, []

    def work(slot, x0):
        try:
            gpu.cuda.set_device(0)
            results[slot] = R.solve(K.rhs(name), x0=x0)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(0, None)), threading.Thread(target=work, args=(1, K.start_vector(name)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert_outcome(results[0], want, "thread 0")
    assert_outcome(results[1], other, "thread 1")
    assert R.info()[4] == 5
    R.free()
    R.free()
    assert not R.k.value


def test_parts_of_another_size_or_kind_are_refused(gpu, pkg):
    F = pkg._ffi
    H = handle_of(pkg, K.matrix("unsym"))
    R = Raw(pkg, gpu, H, "bicgstab")
    small = handle_of(pkg, sp.identity(7, format="csr")).triangular("lower")
    cplx = handle_of(pkg, K.matrix("unsymz")).triangular("lower")
    good = H.triangular("upper")
    assert R.set(small, None, None) == F.SPL_ERROR_dimension_mismatch
    assert R.set(None, None, small) == F.SPL_ERROR_dimension_mismatch
    assert R.set(cplx, None, None) == F.SPL_ERROR_dimension_mismatch
    assert R.L.spl_krylov_set_preconditioner(R.k, H.handle, None, None) == F.SPL_ERROR_invalid_handle  # a matrix is no solver
    assert R.info()[2] == 0  # nothing was set
    assert R.set(None, None, good) == 0 and R.info()[2] == 8
    assert R.set() == 0 and R.info()[2] == 0
    # the solve's own refusals
    b = dev(gpu, K.rhs("unsym"))
    x = gpu.zeros_like(b)
    result = (C.c_int64 * 4)()
    L = R.L
    assert L.spl_krylov_solve_dev(R.k, b.data_ptr(), x.data_ptr(), 0, 1e-8, 0.0, 10, 0, None, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_krylov_solve_dev(R.k, b.data_ptr(), x.data_ptr(), 0, 1e-8, 0.0, -1, 0, result, None, None) == F.SPL_ERROR_n_nonpositive
    assert L.spl_krylov_solve_dev(R.k, b.data_ptr(), x.data_ptr(), 0, -1.0, 0.0, 10, 0, result, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_krylov_solve_dev(R.k, b.data_ptr(), x.data_ptr(), 0, 1e-8, float("nan"), 10, 0, result, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_krylov_solve_dev(R.k, b.data_ptr(), x.data_ptr(), 0, 1e-8, 0.0, 10, -1, result, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_krylov_solve_dev(R.k, None, x.data_ptr(), 0, 1e-8, 0.0, 10, 0, result, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_krylov_solve_dev(R.k, b.data_ptr(), b.data_ptr(), 0, 1e-8, 0.0, 10, 0, result, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_krylov_solve_dev(R.k, b.data_ptr() + 4, x.data_ptr(), 0, 1e-8, 0.0, 10, 0, result, None, None) == F.SPL_ERROR_argument_missing
    R.free()


# ---- 7. the Python layer -----------------------------------------------------------------------------------------------
def host_matrix(pkg, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    return pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)


@pytest.mark.parametrize("method,name", [("cg", "poisson"), ("cg", "hermitian"), ("bicgstab", "unsym"), ("bicgstab", "shifted")])
def test_python_layer_gives_the_bits_of_the_raw_calls(gpu, pkg, method, name):
    S, b = K.matrix(name), np.array(K.rhs(name))
    H = handle_of(pkg, S)
    for kind in (None, "sgs", "ilu0", "jacobi"):
        if kind == "ilu0":
            M = H.ilu0()
        else:
            M = kind
        solver = H.krylov(method, M)
        if kind == "jacobi":  # the layer makes 1 / diag with torch: the yardstick is given what the device was given
            want = K.DRIVERS[method](S, b, K.preconditioner(S, "jacobi", solver.parts[1].cpu().numpy()), None, K.RTOL, 0.0, 2000)
        else:
            want = K.reference(method, name, kind)
        x, res = solver.solve(b, maxiter=2000)
        assert isinstance(x, np.ndarray) and res["converged"] and res["reason_name"] == "converged"
        assert_outcome((x, [res["iterations"], res["reason"]], res["history"]), want, ("solve", kind))
        x, res = solver.solve(b, maxiter=2000, check_every=5)
        assert_outcome((x, [res["iterations"], res["reason"]], res["history"]), want, ("solve, check_every", kind))
        tx, res = solver.solve(dev(gpu, b), maxiter=2000)
        assert tx.is_cuda
        assert_outcome((tx.cpu().numpy(), [res["iterations"], res["reason"]], res["history"]), want, ("tensor", kind))
        inf = solver.info()
        assert inf["n"] == S.shape[0] and inf["solves"] == 3 and inf["complex"] == np.iscomplexobj(S.data)
        assert (inf["T1"], inf["mid"], inf["T2"]) == {None: (False, False, False), "sgs": (True, True, True),
                                                      "ilu0": (True, False, True), "jacobi": (False, True, False)}[kind]
        solver.free()
        solver.free()
    host = host_matrix(pkg, S)
    call = pkg.cg if method == "cg" else pkg.bicgstab
    x, res = call(host, b, M="sgs", maxiter=2000)
    assert_outcome((x, [res["iterations"], res["reason"]], res["history"]), K.reference(method, name, "sgs"), "sparse." + method)
    start = K.reference(method, name, None, start=True)
    x, res = call(host, b, x0=np.array(K.start_vector(name)), maxiter=2000)
    assert_outcome((x, [res["iterations"], res["reason"]], res["history"]), start, "sparse.%s with a start" % method)


def test_vector_dot_dev_of_the_python_layer(gpu, pkg):
    for cplx in (False, True):
        a, b = K.dot_inputs(8229, cplx, seed=3)
        da, db = dev(gpu, a), dev(gpu, b)
        out = gpu.zeros(1, dtype=da.dtype, device="cuda")
        pkg.vector_dot_dev(8229, da.data_ptr(), db.data_ptr(), out.data_ptr(), is_complex=cplx,
                           stream=gpu.cuda.current_stream().cuda_stream)
        gpu.cuda.synchronize()
        assert same_scalar(out.cpu().numpy()[0], K.dot(a, b))
