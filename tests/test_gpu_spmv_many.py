"""spl_matrix_spmv_many_dev (csrc/spmv_many.hip): Y[:, j] = A X[:, j] (+ Y[:, j]) for k column-major vectors, real and
packed-complex handles, and mulM on Complex Double (spl_mulm_z).  The contract is bit-identity: every column equals the
oracle's axpy_ / axpy_z on that column, for rows of any length — the matrix has one row far longer than any chunk of the
kernel, so a wavefront-tree shortcut for long rows would show here."""
import ctypes as C

import numpy as np
import pytest

from helpers import tuple_to_mat

pytestmark = pytest.mark.gpu

NR, NC = 2999, 2500            # 2999 = 46 * 64 + 55: the last wavefront owns a partial group of rows
LONG_ROW, LONG_LEN = 500, 1500  # a row of 1500 stored entries: six chunks of the real kernel, twelve of the complex
EMPTY0, EMPTY1 = 1000, 1080     # 80 empty rows: more than the 64 of one wavefront
KMAX = 70
# The kernel keeps 16 vectors per pass over A, in tiles of 4 (k = 1 and 2 have kernels of their own):
#   1 | 2 | 3 .. 4    the three tile widths;   4 | 5, 8 | 9, 12 | 13   one more tile;
#   16 | 17, 32 | 33  one more pass;  70 = four passes and a rest of 6 (a tile of 4 and one of 2 live vectors)
KS = [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33, 70]


class Case(object):
    pass


@pytest.fixture(scope="module")
def cases(gpu, pkg, O):
    """the matrix (real, and complex on the same pattern), operands and the oracle's results, computed once"""
    rng = np.random.default_rng(2024)
    nz = 40000
    rows, cols = rng.integers(0, NR, nz), rng.integers(0, NC, nz)
    keep = ((rows < EMPTY0) | (rows >= EMPTY1)) & (rows != LONG_ROW)
    rows, cols = rows[keep], cols[keep]
    long_cols = rng.choice(NC, LONG_LEN, replace=False)
    rows = np.concatenate([rows, np.full(LONG_LEN, LONG_ROW)])
    cols = np.concatenate([cols, long_cols])
    re, im = rng.normal(size=len(rows)), rng.normal(size=len(rows))
    Ar = O.compress(NR, NC, rows, cols, re)
    Ai = O.compress(NR, NC, rows, cols, im)  # the same pattern: explicit zeros stay, duplicates add componentwise
    assert np.array_equal(Ar[2], Ai[2]) and np.array_equal(Ar[3], Ai[3])
    lens = np.bincount(Ar[3], minlength=NR)
    assert lens[LONG_ROW] == LONG_LEN and not lens[EMPTY0:EMPTY1].any() and lens[EMPTY0 - 1] and lens[EMPTY1]
    out = {}
    for kind in ("real", "complex"):
        c = Case()
        if kind == "real":
            c.A, c.dtype, c.axpy_ = Ar, np.float64, O.axpy_
            c.X = rng.normal(size=(NC, KMAX))
            c.Y0 = rng.normal(size=(NR, KMAX))
        else:
            c.A, c.dtype, c.axpy_ = (NR, NC, Ar[2], Ar[3], Ar[4] + 1j * Ai[4]), np.complex128, O.axpy_z
            c.X = rng.normal(size=(NC, KMAX)) + 1j * rng.normal(size=(NC, KMAX))
            c.Y0 = rng.normal(size=(NR, KMAX)) + 1j * rng.normal(size=(NR, KMAX))
        c.M = tuple_to_mat(pkg, c.A)
        c.H = pkg.DeviceMatrix.from_csc(c.M) if kind == "real" else pkg.DeviceMatrix.from_csc_complex(c.M)
        c.ref = {False: np.zeros((NR, KMAX), dtype=c.dtype), True: np.zeros((NR, KMAX), dtype=c.dtype)}
        for j in range(KMAX):
            for acc in (False, True):
                y = np.ascontiguousarray(c.Y0[:, j]) if acc else np.zeros(NR, dtype=c.dtype)
                c.axpy_(c.A, np.ascontiguousarray(c.X[:, j]), y)
                c.ref[acc][:, j] = y
        for a in (c.X, c.Y0, c.ref[False], c.ref[True]):
            a.setflags(write=False)
        out[kind] = c
    return out


def run_many(torch, H, X, k, nrows, accumulate, Y0=None, pad=(5, 3)):
    """k vectors through spmv_many_dev with leading dimensions ncols + pad[0], nrows + pad[1]; the padding of X and of Y
    is NaN, and Y's must still be NaN afterwards.  Without `accumulate` Y starts as garbage the call must overwrite.
    Returns Y as an (nrows, k) array."""
    ncols = X.shape[0]
    ldx, ldy = ncols + pad[0], nrows + pad[1]
    tdt = torch.complex128 if np.iscomplexobj(X) else torch.float64
    nan = complex(np.nan, np.nan) if np.iscomplexobj(X) else np.nan
    dX = torch.full((k, ldx), nan, dtype=tdt, device="cuda")
    dX[:, :ncols] = torch.from_numpy(np.ascontiguousarray(X[:, :k].T)).cuda()
    dY = torch.full((k, ldy), nan, dtype=tdt, device="cuda")
    if accumulate:
        dY[:, :nrows] = torch.from_numpy(np.ascontiguousarray(Y0[:, :k].T)).cuda()
    else:
        dY[:, :nrows] = 12345.0
    H.spmv_many_dev(dX.data_ptr(), ldx, dY.data_ptr(), ldy, k, accumulate=accumulate,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dY.cpu().numpy()
    padding = got[:, nrows:].view(np.float64)  # every part of every entry: a complex pair is two doubles
    assert np.all(np.isnan(padding)), "padding of Y was written"
    return got[:, :nrows].T


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("k", KS)
def test_every_column_is_the_oracles_axpy(gpu, cases, kind, k):
    """both accumulate settings, padded leading dimensions with NaN in the padding"""
    c = cases[kind]
    for acc in (False, True):
        got = run_many(gpu, c.H, c.X, k, NR, acc, c.Y0)
        assert got.dtype == c.dtype
        assert np.array_equal(got, c.ref[acc][:, :k]), "k = %d, accumulate = %s" % (k, acc)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("k", [1, 16, 17])
def test_tight_leading_dimensions(gpu, cases, kind, k):
    """ldx = ncols, ldy = nrows: the vectors touch each other"""
    c = cases[kind]
    for acc in (False, True):
        got = run_many(gpu, c.H, c.X, k, NR, acc, c.Y0, pad=(0, 0))
        assert np.array_equal(got, c.ref[acc][:, :k])


@pytest.mark.parametrize("k", [3, 17])
def test_row_block_handle(gpu, pkg, cases, k):
    """a row block reads all of X and writes nrows_local rows: the oracle's rows of that block"""
    c = cases["real"]
    H = pkg.DeviceMatrix.from_csc(c.M, part=1, nparts=3)
    inf = H.info()
    r0, nl = inf["row0"], inf["nrows_local"]
    assert 0 < r0 and 0 < nl and r0 + nl < NR
    for acc in (False, True):
        got = run_many(gpu, H, c.X, k, nl, acc, c.Y0[r0:r0 + nl])
        assert np.array_equal(got, c.ref[acc][r0:r0 + nl, :k])


def test_64bit_row_pointers_against_spmv_dev(gpu, pkg, O, monkeypatch):
    """the product A A of a small matrix, made while SPL_FORCE_PTR64=1 so that the handle really has no 32-bit row
    pointers (a product this small would get them otherwise): the int64_t instantiation of the kernel against one
    spmv_dev per column on the same handle"""
    torch = gpu
    n, k = 3001, 19
    A = pkg.DeviceMatrix.synthetic("random", n, 6)
    monkeypatch.setenv("SPL_FORCE_PTR64", "1")
    AA, _ = A.spgemm(A)
    monkeypatch.delenv("SPL_FORCE_PTR64")
    assert pkg._ffi.lib().spl_umfpack_di_symbolic_dev(AA.handle, C.byref(C.c_void_p())) == -8  # no 32-bit pointers
    X = np.random.default_rng(3).normal(size=(n, k))
    stream = torch.cuda.current_stream().cuda_stream
    per_column = np.zeros((n, k))
    for j in range(k):
        dx = torch.from_numpy(np.ascontiguousarray(X[:, j])).cuda()
        dy = torch.zeros(n, dtype=torch.float64, device="cuda")
        AA.spmv_dev(dx.data_ptr(), dy.data_ptr(), False, stream)
        torch.cuda.synchronize()
        per_column[:, j] = dy.cpu().numpy()
    assert np.array_equal(run_many(torch, AA, X, k, n, False), per_column)
    rp, ci, v = AA.export_csr()  # and against the oracle, row-gather form
    y = np.zeros(n)
    O.csr_gaxpy32(rp.astype(np.int32), ci, v, np.ascontiguousarray(X[:, k - 1]), y)
    assert np.array_equal(per_column[:, k - 1], y)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("bad", [1, 5])
def test_columns_do_not_leak_into_each_other(gpu, cases, kind, bad):
    """+inf and NaN in one vector of X: every other column of Y is the run without them, bit for bit.  k = 6: the
    second tile has two live vectors, and the last one (5) is the one the kernel repeats in the tile's idle slots"""
    c = cases[kind]
    k = 6
    clean = run_many(gpu, c.H, c.X, k, NR, False)
    X = c.X[:, :k].copy()
    X[::50, bad] = np.inf  # (50 columns: the long row stores 3 of every 5, so some of them are met)
    X[1234, bad] = np.nan
    got = run_many(gpu, c.H, X, k, NR, False)
    others = [j for j in range(k) if j != bad]
    assert np.array_equal(got[:, others], clean[:, others])
    assert not np.all(np.isfinite(got[:, bad]))


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_short_rows_equal_k_calls_of_spmv_dev(gpu, pkg, kind):
    """poisson3d m = 12 (7 entries per row at most): the same bits as one spmv_dev per vector, which FEAST relies on"""
    torch = gpu
    H = pkg.DeviceMatrix.synthetic("poisson3d", 12)
    n = 12 ** 3
    rng = np.random.default_rng(8)
    if kind == "real":
        H.optimize()  # as Matrix.device_handle() does: spmv_dev may run on an image of its own
        X = rng.normal(size=(n, 20))
    else:
        H = H.to_complex()
        X = rng.normal(size=(n, 20)) + 1j * rng.normal(size=(n, 20))
    stream = torch.cuda.current_stream().cuda_stream
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dY = torch.zeros_like(dX)
    for j in range(20):
        H.spmv_dev(dX[j].data_ptr(), dY[j].data_ptr(), False, stream)
    torch.cuda.synchronize()
    loop = dY.cpu().numpy().T
    assert np.any(loop != 0)
    for k in (1, 4, 16, 20):
        assert np.array_equal(run_many(torch, H, X, k, n, False), loop[:, :k])


def test_statuses(gpu, pkg, cases):
    torch = gpu
    L = pkg._ffi.lib()
    F = pkg._ffi
    vp = C.c_void_p
    for kind, entry in (("real", 8), ("complex", 16)):
        c = cases[kind]
        h = c.H.handle
        tdt = torch.float64 if kind == "real" else torch.complex128
        dX = torch.zeros((2, NC + 1), dtype=tdt, device="cuda")
        dY = torch.full((2, NR + 1), 3.0, dtype=tdt, device="cuda")
        x, y = dX.data_ptr(), dY.data_ptr()
        call = L.spl_matrix_spmv_many_dev
        not_a_handle = (C.c_char * 512)()
        assert call(None, 1, vp(x), NC, vp(y), NR, 0, None) == F.SPL_ERROR_invalid_handle
        assert call(C.cast(not_a_handle, vp), 1, vp(x), NC, vp(y), NR, 0, None) == F.SPL_ERROR_invalid_handle
        assert call(h, -1, vp(x), NC, vp(y), NR, 0, None) == F.SPL_ERROR_n_nonpositive
        assert call(h, 1, None, NC, vp(y), NR, 0, None) == F.SPL_ERROR_argument_missing
        assert call(h, 1, vp(x), NC, None, NR, 0, None) == F.SPL_ERROR_argument_missing
        assert call(h, 1, vp(x + entry // 2), NC, vp(y), NR, 0, None) == F.SPL_ERROR_argument_missing
        assert call(h, 1, vp(x), NC, vp(y + entry // 2), NR, 0, None) == F.SPL_ERROR_argument_missing
        assert call(h, 2, vp(x), NC - 1, vp(y), NR, 0, None) == F.SPL_ERROR_dimension_mismatch
        assert call(h, 2, vp(x), NC, vp(y), NR - 1, 0, None) == F.SPL_ERROR_dimension_mismatch
        # k == 0: SPL_OK whatever the pointers are, and nothing is written; none of the refused calls wrote either
        assert call(h, 0, None, 0, None, 0, 0, None) == F.SPL_OK
        assert call(h, 0, vp(x), NC, vp(y), NR, 0, None) == F.SPL_OK
        torch.cuda.synchronize()
        assert bool((dY == 3.0).all())
        # k == 1 takes any leading dimension: there is no second vector
        assert call(h, 1, vp(x), 0, vp(y), 0, 0, None) == F.SPL_OK
        torch.cuda.synchronize()
        assert bool((dY[0, :NR] == 0.0).all()) and bool((dY[0, NR:] == 3.0).all()) and bool((dY[1] == 3.0).all())


@pytest.mark.parametrize("k", [1, 5, 16])
def test_mulm_complex(gpu, pkg, O, cases, k):
    """mulM on Complex Double, and a real matrix promoted for a complex operand: one axpy_z per column, bit for bit"""
    c = cases["complex"]
    B = np.ascontiguousarray(c.X[:, :k])
    got = pkg.mulM(c.M, B)
    assert got.dtype == np.complex128 and got.shape == (NR, k)
    assert np.array_equal(got, c.ref[False][:, :k])
    r = cases["real"]
    promoted = (NR, NC, r.A[2], r.A[3], r.A[4].astype(np.complex128))
    want = np.zeros((NR, k), dtype=np.complex128)
    for j in range(k):
        y = np.zeros(NR, dtype=np.complex128)
        O.axpy_z(promoted, np.ascontiguousarray(B[:, j]), y)
        want[:, j] = y
    got = pkg.mulM(r.M, B)
    assert got.dtype == np.complex128 and np.array_equal(got, want)
    # a complex matrix with a real operand is promoted the other way round
    assert np.array_equal(pkg.mulM(c.M, np.ascontiguousarray(r.X[:, :k])),
                          pkg.mulM(c.M, r.X[:, :k].astype(np.complex128)))


def test_mulm_complex_inner_dimension(gpu, pkg, cases):
    c = cases["complex"]
    with pytest.raises(pkg.SparseError) as real_path:
        pkg.mulM(cases["real"].M, np.zeros((NC + 1, 2)))
    with pytest.raises(pkg.SparseError) as complex_path:
        pkg.mulM(c.M, np.zeros((NC + 1, 2), dtype=np.complex128))
    assert str(complex_path.value) == str(real_path.value)
    # and the ABI's own guard, as spl_mulm's
    nr, nc, ap, ai, az = c.M._tuple32()
    F = pkg._ffi
    out = np.zeros(2 * nr)
    st = F.lib().spl_mulm_z(nr, nc, F.p_i32(ap), F.p_i32(ai), F.p_f64(az), nc + 1, 1, F.p_f64(np.zeros(2 * (nc + 1))),
                            F.p_f64(out))
    assert st == F.SPL_ERROR_dimension_mismatch
