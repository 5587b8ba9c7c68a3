"""ILU(0) on device handles (csrc/ilu0.hip): the factor handle, the plan and the two solvers built from it, real and
complex.  The yardstick is the serial IKJ loop of the header restated on Python floats (tests/ilu0_cases.py); the
device result must equal it BIT FOR BIT on every structure and knob setting — NaNs are compared as NaNs only where a
pivot is zero or missing.  The product tests use the standard bound of a length-len recurrence,
(longest row + 2) 2^-53 (|L||U|)_ij."""
import ctypes as C
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ilu0_cases as K
import trisolve_cases as TK

pytestmark = pytest.mark.gpu

HUGE = str(2 ** 30)
KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS")
U53 = 2.0 ** -53
BOTH = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])


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


def values_of(F, S):
    """the values of the factor handle F in S's entry order, after checking that F has S's pattern and value kind"""
    rp, ci, v = F.export_csr()
    assert np.array_equal(rp, S.indptr) and np.array_equal(ci, S.indices), "F's pattern is not A's"
    assert v.dtype == S.data.dtype
    return v


def scipy_of(H):
    inf = H.info()
    rp, ci, v = H.export_csr()
    return sp.csr_matrix((v, ci, rp), shape=(inf["nrows_global"], inf["ncols"]))


def raw_factor(pkg, plan, H):
    """(status, DeviceMatrix or None) of spl_ilu0_factor, without the Python object"""
    f = C.c_void_p(0x1234)
    st = pkg._ffi.lib().spl_ilu0_factor(plan, H.handle, C.byref(f))
    return st, (pkg.DeviceMatrix(f.value) if f.value else None)


# ---- 1. the bits of the serial loop ----------------------------------------------------------------------------------
STRUCTURES = ["poisson40", "tridiagonal", "dense70", "arrow", "blocks", "identity", "strictlower"]


@BOTH
@pytest.mark.parametrize("name", STRUCTURES)
def test_bits_of_the_serial_loop(gpu, pkg, name, cplx):
    S = K.matrix(name, cplx)
    I = handle_of(pkg, S).ilu0()
    inf = I.info()
    lens = np.diff(S.indptr)
    assert (inf["n"], inf["nnz"], inf["longest_row"]) == (S.shape[0], S.nnz, int(lens.max()))
    assert inf["levels"] == max(K.levels_of(S)) + 1 and inf["factorisations"] == 1 and inf["device_bytes"] > 0
    assert I.factors.is_complex == cplx
    got = values_of(I.factors, S)
    if name == "strictlower":
        # every pivot is missing: the real quotients are +-inf and are still compared bit for bit; the complex quotient
        # by 0 :+ 0 is NaN, whose sign and payload differ between CPython's float("nan") and the hardware's, so NaNs
        # are compared as NaNs and everything else by its bits
        assert I.singular and inf["missing_diagonals"] == S.shape[0]
        assert K.nan_or_bits_equal(got, K.reference(name, cplx))
    else:
        assert not I.singular and inf["missing_diagonals"] == 0
        assert K.bits_equal(got, K.reference(name, cplx))
    I.free()
    I.free()


# ---- 2. rows of 1 to 300 entries: every G and rows of several chunks ------------------------------------------------
@BOTH
@pytest.mark.parametrize("small_rows", [None, "1"], ids=["one-narrow-segment", "every-row-a-launch"])
def test_random_rows_of_1_to_300_entries(gpu, pkg, monkeypatch, cplx, small_rows):
    """one row per level (tests/test_ilu0_cpu.py asserts it): by default one workgroup walks all 600 with 64 lanes per
    row; with every level wide each row is a launch whose G is the power of two above its own length, 1 ... 64"""
    if small_rows:
        monkeypatch.setenv("SPL_TRSV_SMALL_ROWS", small_rows)
    S = K.matrix("random", cplx)
    I = handle_of(pkg, S).ilu0()
    inf = I.info()
    assert (inf["levels"], inf["longest_row"]) == (600, 300)
    assert inf["launches"] == (600 if small_rows else 1)
    assert K.bits_equal(values_of(I.factors, S), K.reference("random", cplx))
    I.free()


# ---- 3. the schedule does not show in the bits ------------------------------------------------------------------------
@pytest.mark.parametrize("name,cplx", [("poisson40", False), ("poisson40", True), ("tridiagonal", False),
                                       ("random", True)])
def test_schedule_independence(gpu, pkg, monkeypatch, name, cplx):
    S = K.matrix(name, cplx)
    H = handle_of(pkg, S)
    ref = K.reference(name, cplx)
    seen = set()
    for small in ("1", "8", "64", HUGE):
        for levels in ("1", "5", "1024"):
            monkeypatch.setenv("SPL_TRSV_SMALL_ROWS", small)
            monkeypatch.setenv("SPL_TRSV_SEGMENT_LEVELS", levels)
            I = H.ilu0()  # the knobs are read by the analysis
            inf = I.info()
            seen.add(inf["launches"])
            if small == "1" or levels == "1":
                assert inf["launches"] == inf["levels"]
            if small == HUGE and levels == "1024":
                assert inf["launches"] == -(-inf["levels"] // 1024)
            assert K.bits_equal(values_of(I.factors, S), ref), (small, levels)
            I.free()
    assert len(seen) > 1  # the knobs were read


# ---- 4. patterns without fill: L U = A ---------------------------------------------------------------------------------
def product_bound(S, L, U, P, longest):
    """max over the entries of P - A (the union of both patterns) of |p_ij - a_ij| / (2^-53 (|L||U|)_ij); the test
    asks for at most longest + 2"""
    D = sp.coo_matrix(sp.csr_matrix(P) - sp.csr_matrix(S))
    scale = sp.csr_matrix(abs(L) @ abs(U))
    at = np.asarray(scale[D.row, D.col]).ravel()
    err = np.abs(D.data)
    assert np.all(err <= (longest + 2) * U53 * at), float(np.max(err[at > 0] / at[at > 0]) / U53)
    return float(np.max(err[at > 0] / at[at > 0]) / U53) if np.any(at > 0) else 0.0


@BOTH
@pytest.mark.parametrize("name", ["tridiagonal", "dense70", "arrow"])
def test_no_fill_patterns_multiply_back_to_a(gpu, pkg, name, cplx):
    """tril(F, -1) + I times triu(F), formed with the library's band / lin / SpGEMM on handles, is A within the bound
    of the recurrence, and has nothing outside A's pattern beyond it"""
    S = K.matrix(name, cplx)
    n = S.shape[0]
    I = handle_of(pkg, S).ilu0()
    F = I.factors
    L = F.band(None, -1).lin(1.0, pkg.DeviceMatrix.ident(n, complex=cplx), 1.0)
    Uh = F.triu()
    P, _ = L.spgemm(Uh)
    ratio = product_bound(S, scipy_of(L), scipy_of(Uh), scipy_of(P), I.info()["longest_row"])
    print("%s %s: largest |(L U - A)_ij| / (2^-53 (|L||U|)_ij) = %.3g" % (name, "complex" if cplx else "real", ratio))
    I.free()


# ---- 5. the ILU(0) property: L U agrees with A on A's pattern ------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("name", ["poisson32", "random"])
def test_lu_agrees_with_a_on_the_pattern(gpu, pkg, name, cplx):
    S = K.matrix(name, cplx)
    I = handle_of(pkg, S).ilu0()
    L, U = K.factors_of(S, values_of(I.factors, S))
    P = sp.csr_matrix(L @ U)
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    scale = sp.csr_matrix(abs(L) @ abs(U))
    err = np.abs(np.asarray(P[rows, S.indices]).ravel() - S.data)
    at = np.asarray(scale[rows, S.indices]).ravel()
    ratio = float(np.max(err / at)) / U53
    print("%s %s: largest |(L U)_ij - a_ij| / (2^-53 (|L||U|)_ij) = %.3g" % (name, "complex" if cplx else "real", ratio))
    assert np.all(err <= (I.info()["longest_row"] + 2) * U53 * at), ratio
    I.free()


# ---- 6. into the solves ----------------------------------------------------------------------------------------------------
def yardstick_apply(S, values, op, B):
    F = sp.csr_matrix((values, S.indices, S.indptr), shape=S.shape)
    if op == "N":
        return TK.solve_columns(F, False, False, "N", TK.solve_columns(F, True, True, "N", B))
    return TK.solve_columns(F, True, True, op, TK.solve_columns(F, False, False, op, B))


def run_apply(torch, I, B, trans, in_place):
    n, k = B.shape
    tdt = torch.complex128 if np.iscomplexobj(B) else torch.float64
    ld = n + 3
    dB = torch.zeros((k, ld), dtype=tdt, device="cuda")
    dB[:, :n] = torch.from_numpy(np.array(B.T, order="C")).cuda()
    dX = dB if in_place else torch.full((k, ld), 7.0, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    I.apply_dev(dB.data_ptr(), ld, dX.data_ptr(), ld, k, trans, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return np.asfortranarray(dX.cpu().numpy()[:, :n].T)


@BOTH
def test_apply_dev_is_the_two_serial_solves(gpu, pkg, cplx):
    S = K.matrix("poisson40", cplx)
    I = handle_of(pkg, S).ilu0()
    B = TK.rhs(S.shape[0], 3, cplx)
    for op in ("N", "T", "H") if cplx else ("N", "T"):
        ref = yardstick_apply(S, K.reference("poisson40", cplx), op, B)
        assert np.all(np.isfinite(ref))
        assert K.bits_equal(run_apply(gpu, I, B, op, False), ref), op
        assert K.bits_equal(run_apply(gpu, I, B, op, True), ref), op
        assert K.bits_equal(I.solve(np.asfortranarray(B), op), ref), op
    with pytest.raises(ValueError):
        I.apply_dev(0, 1, 0, 1, 1, "C")
    I.free()


def test_preconditioned_richardson_on_the_device(gpu, pkg):
    """x <- x + M^-1 (b - A x), 30 times, with spmv_dev, apply_dev and torch's vector arithmetic; the same iteration
    in numpy / scipy on the exported factors, for the 5-point Laplacian on a 32 x 32 grid.  The cap of 0.1 is on the
    HOST value: a sanity check of the reference (30 Jacobi steps reach 0.068)"""
    torch = gpu
    S = K.laplacian(32)
    n = S.shape[0]
    A = handle_of(pkg, S)
    I = A.ilu0()
    b = np.random.default_rng(77).standard_normal(n)
    stream = torch.cuda.current_stream().cuda_stream
    db = torch.from_numpy(b).cuda()
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    r = torch.empty_like(x)
    z = torch.empty_like(x)
    for _ in range(30):
        A.spmv_dev(x.data_ptr(), r.data_ptr(), stream=stream)
        torch.sub(db, r, out=r)
        I.apply_dev(r.data_ptr(), n, z.data_ptr(), n, 1, "N", stream)
        x += z
    A.spmv_dev(x.data_ptr(), r.data_ptr(), stream=stream)
    got = float(torch.linalg.norm(db - r) / torch.linalg.norm(db))
    L, U = K.factors_of(S, values_of(I.factors, S))
    xh = np.zeros(n)
    for _ in range(30):
        rh = b - S @ xh
        xh = xh + spla.spsolve_triangular(U, spla.spsolve_triangular(L, rh, lower=True, unit_diagonal=True), lower=False)
    want = float(np.linalg.norm(b - S @ xh) / np.linalg.norm(b))
    print("relative residual after 30 steps: device %.6g, host %.6g" % (got, want))
    assert want < 0.1
    assert abs(got - want) <= 1e-9 * want
    I.free()


# ---- 7. zero and missing pivots -------------------------------------------------------------------------------------------
@BOTH
def test_zero_and_missing_pivots(gpu, pkg, cplx):
    """`both`: a stored 0.0 diagonal in row 5 and no diagonal in row 12, both with dependants.  A pattern that lacks a
    diagonal entry is singular whatever its values are, so good values on the same plan are asked of the full pattern:
    `zero` (the stored 0.0 alone) and `good` share it"""
    F = pkg._ffi
    both, zero, good = K.pivots_cases(cplx)
    H = handle_of(pkg, both)
    assert H.info()["nnz"] == both.nnz  # the stored zero is an entry of the handle
    I = H.ilu0()
    assert I.singular and I.info()["missing_diagonals"] == 1
    st, again = raw_factor(pkg, I.plan, H)
    assert st == F.SPL_WARNING_singular_matrix and again is not None
    ref = K.serial_ilu0(both)
    assert not np.all(np.isfinite(ref.view(np.float64)))  # the yardstick has the inf / NaN pattern
    assert K.nan_or_bits_equal(values_of(I.factors, both), ref)
    assert K.nan_or_bits_equal(values_of(again, both), ref)
    I.free()
    # the stored zero alone, then good values on the same plan
    I = handle_of(pkg, zero).ilu0()
    assert I.singular and I.info()["missing_diagonals"] == 0
    assert K.nan_or_bits_equal(values_of(I.factors, zero), K.serial_ilu0(zero))
    Hg = handle_of(pkg, good)
    st, Fg = raw_factor(pkg, I.plan, Hg)
    assert st == F.SPL_OK
    assert K.bits_equal(values_of(Fg, good), K.serial_ilu0(good))
    I.refactor(Hg)
    assert not I.singular and not I.lower.singular and not I.upper.singular
    I.free()


# ---- 8. refactorisation --------------------------------------------------------------------------------------------------
def test_one_plan_factors_new_values_and_a_complex_handle(gpu, pkg):
    name = "poisson40"
    I = handle_of(pkg, K.matrix(name, False)).ilu0()
    assert K.bits_equal(values_of(I.factors, K.matrix(name, False)), K.reference(name, False))
    for cplx, values in ((False, 1), (True, 0)):
        S = K.matrix(name, cplx, values=values)
        st, Fh = raw_factor(pkg, I.plan, handle_of(pkg, S))
        assert st == pkg._ffi.SPL_OK and Fh.is_complex == cplx
        assert K.bits_equal(values_of(Fh, S), K.reference(name, cplx, values=values)), (cplx, values)
    assert I.info()["factorisations"] == 3
    # refactor: the two solvers answer with the new values, here the complex ones
    S = K.matrix(name, True)
    I.refactor(handle_of(pkg, S))
    assert I.info()["factorisations"] == 4 and I.factors.is_complex and not I.singular
    B = TK.rhs(S.shape[0], 2, True)
    assert K.bits_equal(I.solve(np.asfortranarray(B)), yardstick_apply(S, K.reference(name, True), "N", B))
    assert I.lower.info()["unit"] and not I.upper.info()["unit"] and I.upper.info()["upper"]
    I.free()


# ---- 9. refused inputs ----------------------------------------------------------------------------------------------------
def test_refused_inputs(gpu, pkg):
    F = pkg._ffi
    L = F.lib()
    S = K.matrix("tridiagonal", False, 50)
    H = handle_of(pkg, S)
    # analyze
    R = sp.csc_matrix(K.matrix("dense70", False)[:, :50])
    rect = pkg.DeviceMatrix.from_csc(pkg.Matrix(50, 70, R.indptr, R.indices, R.data))
    D = sp.csc_matrix(K.matrix("dense70", False))
    block = pkg.DeviceMatrix.from_csc(pkg.Matrix(70, 70, D.indptr, D.indices, D.data), part=0, nparts=2)
    for operand, status in ((rect, F.SPL_ERROR_dimension_mismatch), (block, F.SPL_ERROR_invalid_matrix)):
        p = C.c_void_p(0x1234)
        assert L.spl_ilu0_analyze(operand.handle, C.byref(p)) == status and not p.value
        with pytest.raises(pkg.SparseLinearError) as e:
            operand.ilu0()
        assert e.value.status == status
        f = C.c_void_p(0x1234)
        assert L.spl_matrix_ilu0(operand.handle, C.byref(f)) == status and not f.value
    assert L.spl_ilu0_analyze(H.handle, None) == F.SPL_ERROR_argument_missing
    # factor
    I = H.ilu0()
    assert L.spl_ilu0_factor(I.plan, H.handle, None) == F.SPL_ERROR_argument_missing
    other_n = handle_of(pkg, K.matrix("tridiagonal", False, 51))
    fewer = sp.coo_matrix(S)
    keep = ~((fewer.row == 10) & (fewer.col == 11))
    other_nnz = handle_of(pkg, sp.csr_matrix((fewer.data[keep], (fewer.row[keep], fewer.col[keep])), shape=S.shape))
    moved_cols = fewer.col.copy()
    moved_cols[(fewer.row == 10) & (fewer.col == 11)] = 13
    moved = sp.csr_matrix((fewer.data, (fewer.row, moved_cols)), shape=S.shape)
    assert moved.nnz == S.nnz
    block50 = pkg.DeviceMatrix.from_csc(handle_matrix(pkg, S), part=1, nparts=2)
    for wrong in (other_n, other_nnz, handle_of(pkg, moved), block50):
        st, Fh = raw_factor(pkg, I.plan, wrong)
        assert st == F.SPL_ERROR_invalid_matrix and Fh is None
        with pytest.raises(pkg.SparseLinearError):
            I.refactor(wrong)
    # the plan and the object are what they were
    assert I.info()["factorisations"] == 1
    st, Fh = raw_factor(pkg, I.plan, H)
    assert st == F.SPL_OK and K.bits_equal(values_of(Fh, S), K.serial_ilu0(S))
    assert K.bits_equal(values_of(I.factors, S), K.serial_ilu0(S))
    # a freed plan: the pointer is nulled, a second free is harmless
    p = C.c_void_p(I.plan.value)
    I._finalizer.detach()
    L.spl_ilu0_free(C.byref(p))
    assert not p.value
    L.spl_ilu0_free(C.byref(p))


def handle_matrix(pkg, S):
    S = sp.csc_matrix(S)
    S.sort_indices()
    return pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)


# ---- 10. edges ---------------------------------------------------------------------------------------------------------------
def test_matrices_of_no_and_one_row(gpu, pkg):
    F = pkg._ffi
    for cplx in (False, True):
        I = pkg.DeviceMatrix.ident(0, complex=cplx).ilu0()
        inf = I.info()
        assert [inf[k] for k in ("n", "nnz", "levels", "launches", "missing_diagonals", "longest_row")] == [0] * 6
        assert not I.singular and I.factors.info()["nnz"] == 0 and I.factors.is_complex == cplx
        I.free()
    one = sp.csr_matrix(np.array([[-2.5]]))
    I = handle_of(pkg, one).ilu0()
    assert not I.singular and (I.info()["levels"], I.info()["launches"]) == (1, 1)
    assert K.bits_equal(values_of(I.factors, one), np.array([-2.5]))
    assert K.bits_equal(I.solve(np.array([5.0])), np.array([-2.0]))
    I.free()
    empty = pkg.DeviceMatrix.from_csr(1, 1, [0, 0], [], [])
    I = empty.ilu0()
    assert I.singular and I.info()["missing_diagonals"] == 1 and I.factors.info()["nnz"] == 0
    st, _ = raw_factor(pkg, I.plan, empty)
    assert st == F.SPL_WARNING_singular_matrix
    I.free()


@BOTH
def test_four_threads_on_one_plan(gpu, pkg, cplx):
    """different value sets on one pattern, factored concurrently on one plan: each result has its own bits"""
    name = "poisson40"
    mats = [K.matrix(name, cplx, values=v) for v in range(4)]
    handles = [handle_of(pkg, S) for S in mats]
    I = handles[0].ilu0()
    results, errors = {}, []
    start = threading.Barrier(4)

    def work(c):
        try:
            start.wait()
            for rep in range(3):
                st, Fh = raw_factor(pkg, I.plan, handles[c])
                results[(c, rep)] = (st, values_of(Fh, mats[c]))
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(c,)) for c in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 12 and I.info()["factorisations"] == 13
    for (c, rep), (st, v) in results.items():
        assert st == pkg._ffi.SPL_OK and K.bits_equal(v, K.reference(name, cplx, values=c)), (c, rep)
    I.free()


@BOTH
def test_the_one_shot_call_is_analyze_and_factor(gpu, pkg, cplx):
    S = K.matrix("blocks", cplx)
    H = handle_of(pkg, S)
    f = C.c_void_p()
    assert pkg._ffi.lib().spl_matrix_ilu0(H.handle, C.byref(f)) == pkg._ffi.SPL_OK
    one_shot = pkg.DeviceMatrix(f.value)
    I = H.ilu0()
    assert K.bits_equal(values_of(one_shot, S), values_of(I.factors, S))
    assert K.bits_equal(values_of(one_shot, S), K.reference("blocks", cplx))
    # the host-tuple convenience
    J = pkg.ilu0(handle_matrix(pkg, S))
    assert K.bits_equal(values_of(J.factors, S), K.reference("blocks", cplx))
    I.free()
    J.free()
