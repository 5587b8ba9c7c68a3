"""Sparse triangular solves on device handles (csrc/trisolve.hip): T x = b, T^T x = b, T^H x = b, real and complex, k
right-hand sides.  The yardstick is the serial loop of the header restated on Python floats (tests/trisolve_cases.py);
the device result must equal it BIT FOR BIT, on every structure, mode and knob setting — NaNs are compared as NaNs only
where a diagonal is zero.  The residual test at the end uses a derived bound (Higham's, for substitution in any
order), evaluated exactly in fractions."""
import ctypes as C
import threading
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import trisolve_cases as K

pytestmark = pytest.mark.gpu

HUGE = str(2 ** 30)
KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS")


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


def run_solve(torch, T, B, trans="N", pad=(5, 3), in_place=False, stream=None):
    """B (n x k) through solve_dev with leading dimensions n + pad[0], n + pad[1]; the padding rows of B and X hold NaN
    and X's must still hold NaN afterwards, X starts as garbage the call must overwrite.  Returns X as (n, k)"""
    B = np.asarray(B)
    if B.ndim == 1:
        B = B.reshape(-1, 1)
    n, k = B.shape
    cplx = np.iscomplexobj(B)
    tdt = torch.complex128 if cplx else torch.float64
    nan = complex(np.nan, np.nan) if cplx else np.nan
    ldb, ldx = n + pad[0], n + pad[1]
    dB = torch.full((k, ldb), nan, dtype=tdt, device="cuda")
    dB[:, :n] = torch.from_numpy(np.array(B.T, order="C")).cuda()  # (a writable copy)
    if in_place:
        dX, ldx = dB, ldb
    else:
        dX = torch.full((k, ldx), nan, dtype=tdt, device="cuda")
        dX[:, :n] = 12345.0
    torch.cuda.synchronize()
    if stream is None:
        T.solve_dev(dB.data_ptr(), ldb, dX.data_ptr(), ldx, k, trans, torch.cuda.current_stream().cuda_stream)
    else:
        with torch.cuda.stream(stream):
            T.solve_dev(dB.data_ptr(), ldb, dX.data_ptr(), ldx, k, trans, stream.cuda_stream)
        stream.synchronize()
    torch.cuda.synchronize()
    got = dX.cpu().numpy()
    assert np.all(np.isnan(got[:, n:].view(np.float64))), "padding of X was written"
    if not in_place:
        assert K.bits_equal(dB.cpu().numpy()[:, :n], np.ascontiguousarray(B.T)), "B was written"
    return np.asfortranarray(got[:, :n].T)


def solver_for(pkg, name, cplx, upper, unit, with_diag=True):
    H = handle_of(pkg, K.matrix(name, cplx, upper, unit_scaled=unit, with_diag=with_diag))
    T = H.triangular("upper" if upper else "lower", unit)
    H.free()  # the object keeps its own copy: the handle goes before the first solve
    return T


# ---- every structure, both triangles, both value kinds, the three ops, both diagonal modes ------------------------
SMALL_NAMES = [n for n in K.NAMES if n != "random"]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("name", SMALL_NAMES)
def test_bits_of_the_serial_loop(gpu, pkg, name, upper, cplx):
    for unit in (False, True):
        T = solver_for(pkg, name, cplx, upper, unit)
        inf = T.info()
        S = K.matrix(name, cplx, upper, unit_scaled=unit)
        assert (inf["n"], inf["stored"], inf["zero_diagonals"]) == (S.shape[0], S.nnz, 0)
        assert (inf["complex"], inf["upper"], inf["unit"], inf["transposed_built"]) == (cplx, upper, unit, False)
        assert not T.singular and inf["longest_row"] == int(np.max(np.diff(S.indptr)))
        for op in "NTH":
            ref = K.reference(name, cplx, upper, unit, op, 2)
            got = run_solve(gpu, T, K.rhs(S.shape[0], 2, cplx), op)
            assert K.bits_equal(got, ref), (name, upper, cplx, unit, op)
        assert T.info()["transposed_built"]
        T.free()


RANDOM_MODES = [(False, False, "N"), (True, True, "T"), (False, False, "H")]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("upper,unit,op", RANDOM_MODES, ids=["lower-stored-N", "upper-unit-T", "lower-stored-H"])
def test_random_rows_of_1_to_300_entries(gpu, pkg, cplx, upper, unit, op):
    """n = 5000, rows of 1 ... 300 stored entries: rows far longer than a group of 64 lanes, thousands of levels"""
    T = solver_for(pkg, "random", cplx, upper, unit)
    inf = T.info()
    lens = np.diff(K.matrix("random", cplx, False).indptr)  # of the lower triangle; its mirror image has its columns
    assert lens.max() == 300 and lens.min() == 1
    assert inf["longest_row"] == np.diff(K.matrix("random", cplx, upper, unit_scaled=unit).indptr).max() >= 300
    assert inf["levels"] > 300
    got = run_solve(gpu, T, K.rhs(5000, 1, cplx), op)
    assert K.bits_equal(got, K.reference("random", cplx, upper, unit, op, 1))
    T.free()


# ---- right-hand sides: groups of 8, every column the single-column solve ----------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("k", [1, 3, 8, 17])
def test_k_right_hand_sides(gpu, pkg, k, cplx):
    for name, upper, unit, op in (("poisson", False, False, "N"), ("dense70", True, False, "H"),
                                  ("dense70", False, True, "T")):
        T = solver_for(pkg, name, cplx, upper, unit)
        B = K.rhs(T.info()["n"], k, cplx)
        ref = K.reference(name, cplx, upper, unit, op, k)
        assert K.bits_equal(run_solve(gpu, T, B, op), ref)
        assert K.bits_equal(run_solve(gpu, T, B, op, in_place=True), ref)
        assert K.bits_equal(run_solve(gpu, T, B, op, pad=(0, 0)), ref)  # the columns touch each other
        T.free()


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_column_c_is_the_single_column_solve(gpu, pkg, cplx):
    """device against device on the long rows: 17 columns at once (8 + 8 + 1), and each of them alone"""
    for name, op in (("dense200", "N"), ("random", "T")):
        T = solver_for(pkg, name, cplx, False, False)
        n = T.info()["n"]
        B = K.rhs(n, 17, cplx, seed=9)
        many = run_solve(gpu, T, B, op)
        for c in (0, 3, 7, 8, 15, 16):
            assert K.bits_equal(many[:, c:c + 1], run_solve(gpu, T, B[:, c:c + 1], op)), (name, c)
        T.free()


def test_non_default_stream_and_tensors(gpu, pkg):
    torch = gpu
    for cplx in (False, True):
        T = solver_for(pkg, "poisson", cplx, False, False)
        B = K.rhs(1600, 3, cplx)
        ref = K.reference("poisson", cplx, False, False, "N", 3)
        s = torch.cuda.Stream()
        assert K.bits_equal(run_solve(torch, T, B, "N", stream=s), ref)
        # the tensor form: Fortran order in, Fortran order out, on torch's current stream
        with torch.cuda.stream(s):
            b = torch.from_numpy(np.array(B.T, order="C")).cuda().T
            x = T.solve(b)
        s.synchronize()
        assert tuple(x.shape) == (1600, 3) and x.stride(0) == 1
        assert K.bits_equal(np.asfortranarray(x.cpu().numpy()), ref)
        x1 = T.solve(b[:, 1].contiguous())
        torch.cuda.synchronize()
        assert K.bits_equal(x1.cpu().numpy(), np.ascontiguousarray(ref[:, 1]))
        # one column as a 2-D tensor: a slice of a Fortran-ordered tensor is a column, solved; the same slice of a
        # row-major tensor has its entries k apart and is refused like any row-major operand, never read as a column
        xc = T.solve(b[:, 2:3])
        torch.cuda.synchronize()
        assert tuple(xc.shape) == (1600, 1)
        assert K.bits_equal(np.ascontiguousarray(xc.cpu().numpy()[:, 0]), np.ascontiguousarray(ref[:, 2]))
        row_major = b.contiguous()
        assert row_major.stride() == (3, 1)
        for wrong in (row_major, row_major[:, 2:3], row_major[:, 0:1], row_major[:, 1]):  # the last: 1-D, stride 3
            with pytest.raises(pkg.SparseError):
                T.solve(wrong)
        # numpy copies such a slice into a column: the same bits
        xn = T.solve(np.ascontiguousarray(B)[:, 2:3])
        assert xn.shape == (1600, 1) and K.bits_equal(np.ascontiguousarray(xn[:, 0]), np.ascontiguousarray(ref[:, 2]))
        # the numpy form, 1-D and 2-D
        assert K.bits_equal(T.solve(np.asfortranarray(B)), ref)
        assert K.bits_equal(T.solve(np.ascontiguousarray(B[:, 2])), np.ascontiguousarray(ref[:, 2]))
        T.free()
    # the convenience on the host Matrix
    S = sp.csc_matrix(K.matrix("dense70", False))
    M = pkg.Matrix(70, 70, S.indptr, S.indices, S.data)
    x = pkg.solveTriangular(M, np.ascontiguousarray(K.rhs(70, 1, False)[:, 0]), lower=True, trans="T")
    assert K.bits_equal(x, np.ascontiguousarray(K.reference("dense70", False, False, False, "T", 1)[:, 0]))


# ---- the other side of the diagonal is not read --------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_full_matrix_solved_as_lower_and_as_upper(gpu, pkg, cplx):
    A = K.full_matrix(cplx)
    H = handle_of(pkg, A)
    B = K.rhs(400, 3, cplx)
    for uplo, part, cut in (("lower", sp.tril(A), H.tril()), ("upper", sp.triu(A), H.triu())):
        for unit in (False, True):
            Tfull, Tcut = H.triangular(uplo, unit), cut.triangular(uplo, unit)
            assert Tfull.info()["stored"] == Tcut.info()["stored"] == part.nnz
            assert Tfull.info()["levels"] == Tcut.info()["levels"]
            for op in "NTH":
                ref = K.solve_columns(sp.csr_matrix(part), uplo == "lower", unit, op, B)
                got = run_solve(gpu, Tfull, B, op)
                assert K.bits_equal(got, ref), (uplo, unit, op)
                assert K.bits_equal(run_solve(gpu, Tcut, B, op), got)
            Tfull.free()
            Tcut.free()


def test_unit_diagonal_present_or_absent(gpu, pkg):
    for cplx in (False, True):
        with_d = solver_for(pkg, "poisson", cplx, False, True, with_diag=True)
        without = solver_for(pkg, "poisson", cplx, False, True, with_diag=False)
        assert not with_d.singular and not without.singular
        assert with_d.info()["stored"] == without.info()["stored"] + 1600
        B = K.rhs(1600, 2, cplx)
        for op in "NTH":
            ref = K.reference("poisson", cplx, False, True, op, 2)
            assert K.bits_equal(run_solve(gpu, with_d, B, op), ref)
            assert K.bits_equal(run_solve(gpu, without, B, op), ref)


# ---- the schedule does not show in the bits --------------------------------------------------------------------------
SCHEDULES = [{"SPL_TRSV_SMALL_ROWS": "1"}, {"SPL_TRSV_SMALL_ROWS": HUGE},
             {"SPL_TRSV_SMALL_ROWS": HUGE, "SPL_TRSV_SEGMENT_LEVELS": "1"}, {"SPL_TRSV_SEGMENT_LEVELS": "1"},
             {"SPL_TRSV_SMALL_ROWS": "8", "SPL_TRSV_SEGMENT_LEVELS": "5"}]
SCHEDULE_CASES = [("bidiagonal", False, False), ("poisson", False, False), ("poisson", True, True),
                  ("dense70", False, True), ("dense200", True, False), ("arrow", False, False),
                  ("diagonal", False, False), ("random", False, False)]


@pytest.mark.parametrize("name,upper,cplx", SCHEDULE_CASES)
def test_schedule_independence(gpu, pkg, monkeypatch, name, upper, cplx):
    k = 1 if name == "random" else 3
    ops = "N" if name == "random" else "NT" if not cplx else "NH"
    n = K.matrix(name, cplx, upper).shape[0]
    B = K.rhs(n, k, cplx)
    refs = {op: K.reference(name, cplx, upper, False, op, k) for op in ops}
    seen = set()
    for knobs in SCHEDULES:
        for key, value in knobs.items():
            monkeypatch.setenv(key, value)
        T = solver_for(pkg, name, cplx, upper, False)  # the knobs are read by the analysis
        for key in knobs:
            monkeypatch.delenv(key)
        inf = T.info()
        seen.add(inf["launches"])
        if knobs == SCHEDULES[0]:
            assert inf["launches"] == inf["levels"]  # every level wide
        if knobs == SCHEDULES[2]:
            assert inf["launches"] == inf["levels"]  # every level a narrow segment of its own
        if knobs == SCHEDULES[1]:
            assert inf["launches"] == -(-inf["levels"] // 1024)
        for op in ops:
            assert K.bits_equal(run_solve(gpu, T, B, op), refs[op]), (knobs, op)
        T.free()
    assert len(seen) > 1 or name == "diagonal"  # the settings did change the plan


# ---- zero and missing diagonals ----------------------------------------------------------------------------------------
def nan_or_bits_equal(a, b):
    a = np.ascontiguousarray(a).view(np.float64)
    b = np.ascontiguousarray(b).view(np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
def test_zero_and_missing_diagonals(gpu, pkg, cplx, upper):
    S = sp.coo_matrix(K.matrix("small", cplx, upper))
    n = S.shape[0]
    keep = ~((S.row == 12) & (S.col == 12))  # row 12 loses its diagonal entry
    rows, cols, data = S.row[keep], S.col[keep], S.data[keep].copy()
    data[(rows == 40) & (cols == 40)] = 0.0  # row 40 keeps it as a stored zero
    Z = sp.csr_matrix((data, (rows, cols)), shape=(n, n))  # (explicit zeros stay entries)
    H = handle_of(pkg, Z)
    assert H.info()["nnz"] == len(data)  # the stored zero is an entry of the handle
    B = K.rhs(n, 2, cplx)
    T = H.triangular("upper" if upper else "lower")
    assert T.singular and T.info()["zero_diagonals"] == 2
    for op in "NTH":
        ref = K.solve_columns(Z, not upper, False, op, B)
        assert not np.all(np.isfinite(ref))  # the yardstick has the inf / NaN pattern
        got = run_solve(gpu, T, B, op)  # SPL_OK: solve_dev raises on a negative status
        assert nan_or_bits_equal(got, ref), op
    # with a unit diagonal nothing is singular
    U = H.triangular("upper" if upper else "lower", unit=True)
    assert not U.singular and U.info()["zero_diagonals"] == 0


# ---- consistent with the rest of the library: the solve undoes the product -----------------------------------------------
@pytest.mark.parametrize("name", ["poisson", "dense70", "arrow"])
def test_residual_of_solve_after_mulv(gpu, pkg, name):
    """x^ = T.solve(L.mulv(x)):  |b - T x^|_i <= g_i (|T| |x^|)_i with g_i = m u / (1 - m u), m = len_i + 2, u = 2^-53,
    len_i the stored entries of row i — Higham's componentwise bound for substitution in any order (Accuracy and
    Stability of Numerical Algorithms, Theorem 8.5, row by row: len_i - 1 subtractions, the products and the division).
    Both sides are evaluated exactly."""
    S = K.matrix(name, False)
    n = S.shape[0]
    H = handle_of(pkg, S)
    L = H.tril()
    x = np.ascontiguousarray(K.rhs(n, 1, False, seed=3)[:, 0])
    b = L.mulv(x)
    xh = H.triangular("lower").solve(b)
    u = Fraction(1, 2 ** 53)
    X = [Fraction(v) for v in xh.tolist()]
    worst = Fraction(0)
    for i in range(n):
        lo, hi = S.indptr[i], S.indptr[i + 1]
        cols, vals = S.indices[lo:hi].tolist(), [Fraction(v) for v in S.data[lo:hi].tolist()]
        r = Fraction(float(b[i])) - sum((t * X[j] for j, t in zip(cols, vals)), Fraction(0))
        scale = sum((abs(t) * abs(X[j]) for j, t in zip(cols, vals)), Fraction(0))
        m = (hi - lo) + 2
        bound = m * u / (1 - m * u) * scale
        assert abs(r) <= bound, (i, float(abs(r)), float(bound))
        if scale:
            worst = max(worst, abs(r) / (m * u * scale))
    print("largest |b - T x^|_i / (m u (|T||x^|)_i): %.3g" % float(worst))


# ---- refused inputs ----------------------------------------------------------------------------------------------------
def test_refused_inputs(gpu, pkg):
    torch = gpu
    F = pkg._ffi
    L = F.lib()
    S = sp.csc_matrix(K.matrix("dense70", False))
    M = pkg.Matrix(70, 70, S.indptr, S.indices, S.data)
    block = pkg.DeviceMatrix.from_csc(M, part=0, nparts=2)
    with pytest.raises(pkg.SparseLinearError) as e:
        block.triangular()
    assert e.value.status == F.SPL_ERROR_invalid_matrix
    R = sp.csc_matrix(K.matrix("dense70", False)[:, :50])
    rect = pkg.DeviceMatrix.from_csc(pkg.Matrix(50, 70, R.indptr, R.indices, R.data))
    with pytest.raises(pkg.SparseLinearError) as e:
        rect.triangular("upper")
    assert e.value.status == F.SPL_ERROR_dimension_mismatch

    Tr = solver_for(pkg, "dense70", False, False, False)
    Tz = solver_for(pkg, "dense70", True, False, False)
    br, bz = np.ones(70), np.ones(70, dtype=np.complex128)
    for T, wrong in ((Tr, bz), (Tz, br)):
        with pytest.raises(pkg.SparseError):
            T.solve(wrong)
        with pytest.raises(pkg.SparseError):
            T.solve(torch.from_numpy(wrong).cuda())
    with pytest.raises(pkg.SparseError):
        Tr.solve(np.ones(69))
    with pytest.raises(pkg.SparseError):
        Tr.solve(np.ones((70, 2)))  # C order

    buf = torch.zeros(70 * 4 + 8, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(T, op, k, b, ldb, x, ldx):
        return L.spl_trisolve_solve_dev(T.handle, op, k, C.c_void_p(b), ldb, C.c_void_p(x), ldx, stream)

    assert call(Tr, 0, -1, p, 70, p, 70) == F.SPL_ERROR_n_nonpositive
    assert call(Tr, 0, 0, 0, 0, 0, 0) == F.SPL_OK  # k == 0: nothing is looked at
    assert call(Tr, 3, 1, p, 70, p, 70) == F.SPL_ERROR_argument_missing
    assert call(Tr, -1, 1, p, 70, p, 70) == F.SPL_ERROR_argument_missing
    assert call(Tr, 0, 1, 0, 70, p, 70) == F.SPL_ERROR_argument_missing
    assert call(Tr, 0, 1, p, 70, 0, 70) == F.SPL_ERROR_argument_missing
    assert call(Tr, 0, 1, p + 4, 70, p, 70) == F.SPL_ERROR_argument_missing  # off the 8-byte grid
    assert call(Tz, 0, 1, p + 8, 70, p, 70) == F.SPL_ERROR_argument_missing  # a complex entry is 16 bytes
    assert call(Tz, 0, 1, p, 70, p + 8, 70) == F.SPL_ERROR_argument_missing
    assert call(Tr, 0, 2, p, 69, p, 70) == F.SPL_ERROR_dimension_mismatch
    assert call(Tr, 0, 2, p, 70, p, 69) == F.SPL_ERROR_dimension_mismatch
    assert call(Tr, 0, 1, p, 0, p, 0) == F.SPL_OK  # one column: the leading dimensions are not used
    torch.cuda.synchronize()
    assert not buf.cpu().numpy()[70:].any()  # nothing beyond row n

    # a freed object: the pointer is nulled, a second free is harmless, a solve on it is an invalid handle
    t = C.c_void_p(Tr.handle.value)
    Tr._finalizer.detach()
    L.spl_trisolve_free(C.byref(t))
    assert not t.value
    L.spl_trisolve_free(C.byref(t))
    assert L.spl_trisolve_solve_dev(t, 0, 1, C.c_void_p(p), 70, C.c_void_p(p), 70, stream) == F.SPL_ERROR_invalid_handle
    Tz.free()
    Tz.free()
    with pytest.raises(pkg.SparseLinearError):
        Tz.solve(bz)


def test_a_matrix_without_rows(gpu, pkg):
    for cplx in (False, True):
        T = pkg.DeviceMatrix.diag_dev(0, complex=cplx).triangular("upper")
        inf = T.info()
        assert (inf["n"], inf["stored"], inf["levels"], inf["launches"], inf["zero_diagonals"]) == (0, 0, 0, 0, 0)
        assert not T.singular and inf["complex"] == cplx
        T.solve_dev(0, 0, 0, 0, 3, "T")  # n == 0: SPL_OK, nothing is looked at
        x = T.solve(np.zeros(0, dtype=np.complex128 if cplx else np.float64), "H")
        assert x.shape == (0,)
        T.free()


# ---- several host threads on one object ----------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_four_threads_on_one_object(gpu, pkg, cplx):
    """different right-hand sides, both ops; the object is fresh, so the first transposed solves race for the lazy build"""
    name = "poisson"
    T = solver_for(pkg, name, cplx, False, False)
    B = K.rhs(1600, 4, cplx)
    tr = "H" if cplx else "T"
    refs = {op: K.reference(name, cplx, False, False, op, 4) for op in ("N", tr)}
    results, errors = {}, []
    start = threading.Barrier(4)

    def work(c):
        try:
            b = np.ascontiguousarray(B[:, c])
            start.wait()
            for op in ((tr, "N") if c % 2 == 0 else ("N", tr)) * 3:
                results[(c, op)] = T.solve(b, op)
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(c,)) for c in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for (c, op), x in results.items():
        assert K.bits_equal(x, np.ascontiguousarray(refs[op][:, c])), (c, op)
    assert T.info()["transposed_built"]
