"""Taking a device handle apart: spl_matrix_submatrix (windows) and spl_matrix_select (rows and columns by index),
their Python mirrors and the host route sparse.subMatrix.

Expected values come from numpy on the input arrays (np_window, np_select below), from the CPU oracle for the
products that consume a result (O.axpy, O.lin), or from a round trip through the inverse (DeviceMatrix.assemble);
none from the library under test.  Comparisons are bit for bit: doubles are viewed as uint64.

Base matrices: a rectangular real matrix of 6 007 x 4 099 with about 60 000 entries (mean row length 10), empty rows at
both ends and in the middle, one row of 300 entries (more than 64 lanes, more than one step of a group), values that
are rounding-sensitive doubles salted with -0.0, +inf, -inf and a NaN with a payload; a complex copy of it with its own
imaginary parts; and narrow matrices with mean row lengths of about 1, 2, 3, 7, 25 and 100, which together with the base
make the host choose every group width G = 1, 2, 4 ... 64 in the length passes and in the copy passes."""
import collections
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NR, NC = 6007, 4099
EMPTY_ROWS = (0, 1, 2001, 2002, 2003, NR - 2, NR - 1)
LONG_ROW, LONG_LEN = 3000, 300
ROW_CUTS, COL_CUTS = (0, 1000, 4501, NR), (0, 1001, 3003, NC)  # no multiple of 64 among the inner cuts
NAN_PAYLOAD = np.array([0x7FF80000DEADBEEF], dtype=np.uint64).view(np.float64)[0]
NAN_PAYLOAD_IM = np.array([0xFFF8000000C0FFEE], dtype=np.uint64).view(np.float64)[0]

# an nrows x ncols matrix as CSR arrays with ascending columns inside every row
Csr = collections.namedtuple("Csr", "nrows ncols rp ci v")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


# ---- numpy on the input arrays: the expected values ----------------------------------------------------------------

def csr_from_keys(nrows, ncols, keys, v):
    keys = np.asarray(keys, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    rows = keys[order] // ncols
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))]).astype(np.int64)
    return Csr(nrows, ncols, rp, (keys[order] % ncols).astype(np.int32), np.ascontiguousarray(np.asarray(v)[order]))


def row_ids(t):
    return np.repeat(np.arange(t.nrows, dtype=np.int64), np.diff(t.rp))


def np_window(t, r0, c0, nr, nc):
    a, b = int(t.rp[r0]), int(t.rp[r0 + nr])
    ci, v = t.ci[a:b].astype(np.int64), t.v[a:b]
    rows = np.repeat(np.arange(nr, dtype=np.int64), np.diff(t.rp[r0:r0 + nr + 1]))
    keep = (ci >= c0) & (ci < c0 + nc)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=nr))]).astype(np.int64)
    return Csr(nr, nc, rp, (ci[keep] - c0).astype(np.int32), np.ascontiguousarray(v[keep]))


def np_select(t, I, J):
    I = np.arange(t.nrows, dtype=np.int64) if I is None else np.asarray(I, dtype=np.int64)
    J = np.arange(t.ncols, dtype=np.int64) if J is None else np.asarray(J, dtype=np.int64)
    cmap = np.full(t.ncols, -1, dtype=np.int64)
    cmap[J] = np.arange(len(J))
    lens = np.diff(t.rp)[I]
    start_out = np.concatenate([[0], np.cumsum(lens)])[:-1]
    src = np.repeat(t.rp[I] - start_out, lens) + np.arange(int(lens.sum()), dtype=np.int64)  # source positions, row by row
    rows = np.repeat(np.arange(len(I), dtype=np.int64), lens)
    newc = cmap[t.ci[src]]
    keep = newc >= 0
    rows, newc, v = rows[keep], newc[keep], t.v[src][keep]
    order = np.lexsort((newc, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(I)))]).astype(np.int64)
    return Csr(len(I), len(J), rp, newc[order].astype(np.int32), np.ascontiguousarray(v[order]))


def np_csc(t):
    """(colptr, rowidx, values): rows ascending inside every column"""
    rows = row_ids(t)
    order = np.lexsort((rows, t.ci))
    cp = np.concatenate([[0], np.cumsum(np.bincount(t.ci, minlength=t.ncols))]).astype(np.int64)
    return cp, rows[order], t.v[order]


# ---- the base matrices ----------------------------------------------------------------------------------------------

def make_base():
    rng = np.random.default_rng(20_26)
    keys = np.unique(rng.integers(0, NR, 60_500) * NC + rng.integers(0, NC, 60_500))
    keys = keys[~np.isin(keys // NC, EMPTY_ROWS + (LONG_ROW,))]
    keys = np.concatenate([keys, LONG_ROW * NC + rng.choice(NC, LONG_LEN, replace=False)])
    v = rng.standard_normal(len(keys)) * 10.0 ** rng.integers(-3, 4, len(keys))  # rounding-order sensitive
    t = csr_from_keys(NR, NC, keys, v)
    v = t.v.copy()
    # the salt: at most one non-finite value per row, so that a product with a finite vector never meets inf - inf or
    # two NaNs, and the first entries of rows spread over the matrix, the long row among them
    firsts = t.rp[:-1][np.diff(t.rp) > 0]
    for k, value in ((5, -0.0), (700, np.inf), (1500, -0.0), (2500, -np.inf), (3500, NAN_PAYLOAD), (4200, -0.0)):
        v[firsts[k]] = value
    v[t.rp[LONG_ROW] + 150] = -0.0
    return t._replace(v=v)


def make_complex(t):
    rng = np.random.default_rng(7)
    im = rng.standard_normal(len(t.v)) * 10.0 ** rng.integers(-3, 4, len(t.v))
    im[::977] = -0.0
    im[12345] = NAN_PAYLOAD_IM
    z = np.empty(len(t.v), dtype=np.complex128)
    z.real, z.imag = t.v, im
    return t._replace(v=z)


NARROW = {"mean1": (3001, 517, 0.9), "mean2": (1501, 517, 1.8), "mean3": (2003, 517, 3.2), "mean7": (1201, 701, 7.0),
          "mean25": (601, 701, 25.0), "mean100": (301, 1031, 100.0)}


def make_narrow(name):
    nrows, ncols, mean = NARROW[name]
    rng = np.random.default_rng(len(name) + nrows)
    k = int(nrows * mean)
    keys = np.unique(rng.integers(0, nrows, k + k // 8) * ncols + rng.integers(0, ncols, k + k // 8))
    keys = rng.permutation(keys)[:k]
    return csr_from_keys(nrows, ncols, keys, rng.standard_normal(k))


@pytest.fixture(scope="module")
def base():
    t = make_base()
    out = {"real": t, "complex": make_complex(t)}
    out.update((name, make_narrow(name)) for name in NARROW)
    return out


def test_base_matrices_are_what_the_tests_assume(base):
    t = base["real"]
    lens = np.diff(t.rp)
    assert (t.nrows, t.ncols) == (NR, NC) and 55_000 < len(t.ci) < 65_000
    assert all(lens[r] == 0 for r in EMPTY_ROWS) and lens[LONG_ROW] == LONG_LEN == lens.max()
    inside = np.ones(len(t.ci), dtype=bool)
    inside[t.rp[:-1][lens > 0]] = False
    assert np.all(np.diff(t.ci.astype(np.int64))[inside[1:]] > 0)  # strictly ascending inside every row
    nonfinite = np.bincount(row_ids(t)[~np.isfinite(t.v)], minlength=NR)
    assert nonfinite.max() == 1 and nonfinite.sum() == 3 and np.isnan(t.v).sum() == 1
    assert np.sum(np.signbit(t.v) & (t.v == 0)) == 4
    assert all(c % 64 for c in ROW_CUTS[1:-1] + COL_CUTS[1:-1])
    z = base["complex"]
    assert z.v.dtype == np.complex128 and same_bits(z.v.real, t.v) and np.isnan(z.v.imag).sum() == 1
    # smallest power of two >= the mean row length: the lanes a row gets in the passes that walk source rows
    groups = {name: 1 << int(np.ceil(np.log2(max(len(m.ci) / m.nrows, 1.0)))) for name, m in base.items()}
    assert sorted(set(min(g, 64) for g in groups.values())) == [1, 2, 4, 8, 16, 32, 64], groups


# ---- handles in, arrays out -------------------------------------------------------------------------------------------

def handle(torch, pkg, t):
    """the handle of a Csr through the device-array import: values are moved as bits"""
    cplx = t.v.dtype == np.complex128
    rp = torch.from_numpy(np.ascontiguousarray(t.rp, dtype=np.int64)).cuda()
    ci = torch.from_numpy(np.ascontiguousarray(t.ci, dtype=np.int64)).cuda()
    v = torch.from_numpy(np.ascontiguousarray(t.v)).cuda()
    torch.cuda.synchronize()
    n = len(t.ci)
    return pkg.DeviceMatrix.from_csr_dev(t.nrows, t.ncols, rp.data_ptr(), ci.data_ptr() if n else 0,
                                         v.data_ptr() if n else 0, index_width=8, complex=cplx)


@pytest.fixture(scope="module")
def handles(gpu, pkg, base):
    return {name: handle(gpu, pkg, t) for name, t in base.items()}


def export_csc_dev(torch, H):
    inf = H.info()
    nnz, cplx = inf["nnz"], H.is_complex
    cp = torch.full((inf["ncols"] + 1,), -1, dtype=torch.int64, device="cuda")
    ri = torch.full((max(nnz, 1),), -1, dtype=torch.int64, device="cuda")
    v = torch.zeros(max(nnz, 1), dtype=torch.complex128 if cplx else torch.float64, device="cuda")
    torch.cuda.synchronize()
    H.export_csc_dev(cp.data_ptr(), ri.data_ptr(), v.data_ptr(), index_width=8)
    return cp.cpu().numpy(), ri.cpu().numpy()[:nnz], v.cpu().numpy()[:nnz]


def assert_is(torch, H, t, csc=True):
    """H holds exactly t: dimensions, pointers, indices and value bits, through export_csr and export_csc_dev"""
    inf = H.info()
    assert (inf["nrows_global"], inf["ncols"], inf["row0"], inf["nrows_local"], inf["nnz"]) == \
        (t.nrows, t.ncols, 0, t.nrows, len(t.ci))
    assert H.is_complex == (t.v.dtype == np.complex128)
    rp, ci, v = H.export_csr()
    assert np.array_equal(rp, t.rp) and np.array_equal(ci, t.ci)
    assert v.dtype == t.v.dtype and same_bits(v, t.v)
    if csc:
        cp, ri, cv = export_csc_dev(torch, H)
        want = np_csc(t)
        assert np.array_equal(cp, want[0]) and np.array_equal(ri, want[1]) and same_bits(cv, want[2])


# ---- 1. windows against numpy ---------------------------------------------------------------------------------------

def boundary_windows(t):
    """column ranges whose ends each coincide with a stored column, with the column after a stored one, and fall in a
    gap, read off row 3001 (about ten entries, all three kinds of neighbourhood exist in 4 099 columns)"""
    row = 3001
    cols = t.ci[t.rp[row]:t.rp[row + 1]].astype(np.int64)
    assert len(cols) >= 6
    stored = set(cols.tolist())
    on = [int(c) for c in cols]
    after = [int(c) + 1 for c in cols if int(c) + 1 not in stored]
    gap = [int(c) + 2 for c in cols if int(c) + 1 not in stored and int(c) + 2 not in stored and int(c) + 2 < NC]
    out = []
    for lo, hi in ((on[1], on[4]), (after[1], after[4]), (gap[1], gap[4]), (on[0], gap[3]), (gap[0], after[5])):
        out.append((2900, lo, 200, hi - lo))
    return out


def window_cases(t):
    long_cols = t.ci[t.rp[LONG_ROW]:t.rp[LONG_ROW + 1]].astype(np.int64)
    stored = (3001, int(t.ci[t.rp[3001]]))
    unstored = (3001, int(t.ci[t.rp[3001]]) + 1)
    assert unstored[1] not in t.ci[t.rp[3001]:t.rp[3002]]
    cases = [(0, 0, NR, NC),                      # the whole matrix
             (1000, 0, 1002, NC), (0, 0, 1000, NC), (2002, 0, NR - 2002, NC),  # nc == ncols: nothing is searched
             (LONG_ROW, int(long_cols[40]), 1, int(long_cols[250] - long_cols[40])),  # inside the 300-entry row only
             (LONG_ROW, 0, 1, NC), (LONG_ROW - 3, 1, 7, NC - 2),
             (1000, 17, 0, 300), (1000, 17, 300, 0), (NR, NC, 0, 0), (2001, 0, 3, NC), (2001, 100, 3, 1000),  # nothing kept
             stored + (1, 1), unstored + (1, 1),
             (1000, 5, 1002, 3995), (3, 1001, 4498, 2002)]
    return cases + boundary_windows(t)


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_windows_against_numpy(gpu, base, handles, kind):
    t, H = base[kind], handles[kind]
    for r0, c0, nr, nc in window_cases(base["real"]):
        want = np_window(t, r0, c0, nr, nc)
        assert_is(gpu, H.submatrix(r0, c0, nr, nc), want)
    # the window holding no entry holds none, the one on a stored entry holds that entry
    r, c = 3001, int(t.ci[t.rp[3001]])
    one = H.submatrix(r, c, 1, 1).export_csr()
    assert len(one[1]) == 1 and same_bits(one[2], t.v[t.rp[r]:t.rp[r] + 1])
    assert H.submatrix(r, c + 1, 1, 1).info()["nnz"] == 0


@pytest.mark.parametrize("name", list(NARROW))
def test_windows_of_narrow_matrices(gpu, base, handles, name):
    """every group width in the length pass (source row length) and in the copy pass (kept row length)"""
    t, H = base[name], handles[name]
    for r0, c0, nr, nc in ((0, 0, t.nrows, t.ncols), (7, 0, t.nrows - 70, t.ncols), (3, 1, t.nrows - 5, t.ncols - 2),
                           (65, t.ncols // 4, t.nrows - 130, t.ncols // 2), (1, t.ncols // 3, t.nrows - 1, t.ncols // 4),
                           (100, 5, 129, t.ncols // 16)):
        assert_is(gpu, H.submatrix(r0, c0, nr, nc), np_window(t, r0, c0, nr, nc), csc=False)


# ---- 2. round trip with the inverse ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["real", "complex"])
def test_grid_of_windows_assembles_to_the_matrix(gpu, pkg, base, handles, kind):
    t, H = base[kind], handles[kind]
    blocks, ro, co = [], [], []
    for i in range(3):
        for j in range(3):
            blocks.append(H.submatrix(ROW_CUTS[i], COL_CUTS[j], ROW_CUTS[i + 1] - ROW_CUTS[i], COL_CUTS[j + 1] - COL_CUTS[j]))
            ro.append(ROW_CUTS[i])
            co.append(COL_CUTS[j])
    assert_is(gpu, pkg.DeviceMatrix.assemble(blocks, ro, co, NR, NC), t)
    order = [4, 8, 0, 2, 6, 1, 3, 5, 7]  # the assembly does not depend on the order of its blocks
    assert_is(gpu, pkg.DeviceMatrix.assemble([blocks[k] for k in order], [ro[k] for k in order], [co[k] for k in order],
                                             NR, NC), t, csc=False)
    cols = [H.submatrix(0, COL_CUTS[j], NR, COL_CUTS[j + 1] - COL_CUTS[j]) for j in range(3)]
    assert_is(gpu, pkg.DeviceMatrix.hcat(cols), t, csc=False)
    rows = [H.submatrix(ROW_CUTS[i], 0, ROW_CUTS[i + 1] - ROW_CUTS[i], NC) for i in range(3)]
    assert_is(gpu, pkg.DeviceMatrix.vcat(rows), t, csc=False)


# ---- 3. select against numpy ----------------------------------------------------------------------------------------

def select_cases():
    rng = np.random.default_rng(99)
    I_rep = np.concatenate([rng.integers(0, NR, 700), [LONG_ROW, LONG_ROW, 0, NR - 1, 3500, 3500]])  # repeats
    I_desc = np.arange(NR - 1, -1, -3)
    J_asc = np.arange(1001, 3003)
    J_sub = np.sort(rng.choice(NC, 1500, replace=False))
    return {
        "rows_repeat_cols_all": (I_rep, None),
        "rows_descend_cols_ascend": (I_desc, J_sub),
        "cols_reversed": (None, np.arange(NC)[::-1].copy()),
        "cols_random_permutation": (I_rep, rng.permutation(NC)),
        "cols_random_subset_unordered": (I_desc, rng.permutation(J_sub)),
        "rows_all_cols_all": (None, None),
        "cols_range_only": (None, J_asc),
        "rows_range_only": (np.arange(1000, 4501), None),
        "no_rows": (np.zeros(0, dtype=np.int64), J_sub),
        "no_cols": (I_rep, np.zeros(0, dtype=np.int64)),
        "symmetric_window": (np.arange(1000, 3003), J_asc),
    }


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_select_against_numpy(gpu, base, handles, kind, width):
    torch = gpu
    t, H = base[kind], handles[kind]
    dt = torch.int32 if width == 4 else torch.int64
    for name, (I, J) in select_cases().items():
        dI = None if I is None else torch.from_numpy(I).to(dt).cuda()
        dJ = None if J is None else torch.from_numpy(J).to(dt).cuda()
        assert_is(torch, H.select(dI, dJ), np_select(t, I, J), csc=name in ("cols_random_permutation", "rows_all_cols_all"))


def test_ascending_columns_equal_the_window(gpu, base, handles):
    """J ascending takes the no-sort path and must be the window of the same range; rows 1000 .. 3002 likewise"""
    for kind in ("real", "complex"):
        t, H = base[kind], handles[kind]
        want = np_window(t, 1000, 1001, 2003, 2002)
        assert_is(gpu, H.select(np.arange(1000, 3003), np.arange(1001, 3003)), want, csc=False)
        assert_is(gpu, H.submatrix(1000, 1001, 2003, 2002), want, csc=False)
        assert_is(gpu, H.select(None, np.arange(1001, 3003)), np_window(t, 0, 1001, NR, 2002), csc=False)
        assert_is(gpu, H.select(np.arange(1000, 3003), None), np_window(t, 1000, 0, 2003, NC), csc=False)
        assert_is(gpu, H.select(None, None), t, csc=False)  # a copy of A


@pytest.mark.parametrize("name", list(NARROW))
def test_select_of_narrow_matrices(gpu, base, handles, name):
    """every group width in the count pass and in the ballot of the copy pass, sorted and unsorted columns"""
    t, H = base[name], handles[name]
    rng = np.random.default_rng(t.nrows)
    I = rng.integers(0, t.nrows, t.nrows + 37)
    J = rng.permutation(t.ncols)[: (2 * t.ncols) // 3]
    for rows, cols in ((I, J), (I, np.sort(J)), (None, J), (I, None), (rng.permutation(t.nrows), rng.permutation(t.ncols))):
        assert_is(gpu, H.select(rows, cols), np_select(t, rows, cols), csc=False)


def test_complex_values_follow_their_indices_through_the_sort(gpu, pkg):
    """value = (column, row) on every entry: after a selection by permutations each value still names its source"""
    torch = gpu
    rng = np.random.default_rng(5)
    t = make_narrow("mean25")
    z = np.empty(len(t.ci), dtype=np.complex128)
    z.real, z.imag = t.ci, row_ids(t)
    H = handle(torch, pkg, t._replace(v=z))
    p, q = rng.permutation(t.nrows), rng.permutation(t.ncols)
    rp, ci, v = H.select(p, q).export_csr()
    rows = np.repeat(np.arange(t.nrows), np.diff(rp))
    assert np.array_equal(v.real, q[ci]) and np.array_equal(v.imag, p[rows])
    assert np.array_equal(np.diff(rp), np.diff(t.rp)[p])


def raw_select(pkg, H, nI, dI, nJ, dJ, width):
    h, bad = C.c_void_p(0x1234), C.c_int64(-1)
    st = pkg._ffi.lib().spl_matrix_select(H.handle, nI, None if dI is None else C.c_void_p(dI.data_ptr()), nJ,
                                          None if dJ is None else C.c_void_p(dJ.data_ptr()), width, C.byref(h), C.byref(bad))
    out = pkg.DeviceMatrix(h.value) if st == 0 and h.value else None
    return st, h.value, bad.value, out


def test_an_eight_byte_index_is_checked_before_it_is_narrowed(gpu, pkg, handles):
    torch = gpu
    F = pkg._ffi
    H = handles["real"]
    J = torch.arange(0, 40, dtype=torch.int64, device="cuda")
    J[11] = 2 ** 32 + 3  # not column 3
    I = torch.arange(0, 25, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert raw_select(pkg, H, 25, I, 40, J, 8)[:3] == (F.SPL_ERROR_index_out_of_bounds, None, 11)
    I[9] = 2 ** 32 + 5
    torch.cuda.synchronize()
    assert raw_select(pkg, H, 25, I, 40, J, 8)[:3] == (F.SPL_ERROR_index_out_of_bounds, None, 9)
    I[9], J[11] = -(2 ** 32) + 5, 11
    torch.cuda.synchronize()
    assert raw_select(pkg, H, 25, I, 40, J, 8)[:3] == (F.SPL_ERROR_index_out_of_bounds, None, 9)


# ---- 4. refusals on a real handle, in the header's order -------------------------------------------------------------

def raw_submatrix(pkg, H, r0, c0, nr, nc):
    h = C.c_void_p(0x1234)
    st = pkg._ffi.lib().spl_matrix_submatrix(H.handle, r0, c0, nr, nc, C.byref(h))
    assert st == 0 or not h.value  # *HC is cleared whenever the call is refused
    return st


def test_submatrix_refusals(gpu, pkg, base, handles):
    F = pkg._ffi
    H = handles["real"]
    for args in ((-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1), (0, 0, 1, -1), (-1, 0, NR + 5, 1)):  # negative before the guards
        assert raw_submatrix(pkg, H, *args) == F.SPL_ERROR_n_nonpositive
    for args in ((0, 0, NR + 1, 1), (1, 0, NR, NC), (NR, 0, 1, 1), (0, 0, 1, NC + 1), (0, 1, NR, NC), (0, NC, 0, 1),
                 (2 ** 62, 0, 2 ** 62, 1), (0, 2 ** 63 - 1, 1, 2 ** 63 - 1)):
        assert raw_submatrix(pkg, H, *args) == F.SPL_ERROR_dimension_mismatch
    assert raw_submatrix(pkg, H, 1, 0, NR - 1, NC) == 0 and raw_submatrix(pkg, H, NR, NC, 0, 0) == 0
    # a row block: after the guards (which are made against the global row count)
    t = base["real"]
    a, b = int(t.rp[1000]), int(t.rp[2002])
    blk = pkg.DeviceMatrix.from_csr(NR, NC, t.rp[1000:2003] - a, t.ci[a:b], t.v[a:b], row0=1000)
    assert raw_submatrix(pkg, blk, 1000, 0, 10, 10) == F.SPL_ERROR_argument_missing
    assert raw_submatrix(pkg, blk, 0, 0, NR + 1, 10) == F.SPL_ERROR_dimension_mismatch
    assert raw_submatrix(pkg, blk, -1, 0, NR + 1, 10) == F.SPL_ERROR_n_nonpositive
    assert F.lib().spl_matrix_submatrix(H.handle, -1, 0, NR + 1, 1, None) == F.SPL_ERROR_argument_missing
    with pytest.raises(F.SparseLinearError):
        H.submatrix(0, 0, NR + 1, 1)


def test_select_refusals(gpu, pkg, base, handles):
    torch = gpu
    F = pkg._ffi
    H = handles["real"]
    I = torch.arange(0, 20, dtype=torch.int64, device="cuda")
    J = torch.arange(100, 130, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def refused(*args):
        st, h, bad, _ = raw_select(pkg, H, *args)
        assert not h  # *HC is cleared each time
        return st, bad

    assert raw_select(pkg, H, 20, I, 30, J, 8)[0] == 0
    assert refused(-1, I, 30, J, 8)[0] == F.SPL_ERROR_n_nonpositive
    assert refused(20, I, -1, J, 3)[0] == F.SPL_ERROR_n_nonpositive        # before the width
    assert refused(2 ** 31, I, 30, J, 3)[0] == F.SPL_ERROR_index_overflow  # before the width
    assert refused(20, I, 2 ** 31, J, 8)[0] == F.SPL_ERROR_index_overflow
    for width in (3, 0, 16):
        assert refused(20, I, 30, J, width)[0] == F.SPL_ERROR_argument_missing
    assert refused(20, I[1:].view(torch.int32)[1:], 30, J, 8)[0] == F.SPL_ERROR_argument_missing  # 4 bytes off an 8-byte grid
    assert refused(NR - 1, None, 30, J, 8)[0] == F.SPL_ERROR_dimension_mismatch   # all rows, but another count
    assert refused(20, I, NC + 1, None, 8)[0] == F.SPL_ERROR_dimension_mismatch
    assert refused(NR - 1, None, 30, J, 3)[0] == F.SPL_ERROR_argument_missing     # the width comes first
    assert F.lib().spl_matrix_select(H.handle, 20, C.c_void_p(I.data_ptr()), 30, C.c_void_p(J.data_ptr()), 8, None,
                                     None) == F.SPL_ERROR_argument_missing
    # a repeated column
    Jr = J.clone()
    Jr[17] = Jr[4]
    torch.cuda.synchronize()
    assert refused(20, I, 30, Jr, 8) == (F.SPL_ERROR_invalid_matrix, -1)
    # I out of range at 5 and J out of range at 7 in the same call: I is checked first
    Ib, Jb = I.clone(), J.clone()
    Ib[5], Ib[12], Jb[7] = NR, -1, NC
    torch.cuda.synchronize()
    assert refused(20, Ib, 30, Jb, 8) == (F.SPL_ERROR_index_out_of_bounds, 5)
    assert refused(20, I, 30, Jb, 8) == (F.SPL_ERROR_index_out_of_bounds, 7)
    Jb[7], Jb[3] = Jb[6], -1  # out of range before repeated
    torch.cuda.synchronize()
    assert refused(20, I, 30, Jb, 8) == (F.SPL_ERROR_index_out_of_bounds, 3)
    st = F.lib().spl_matrix_select(H.handle, 20, C.c_void_p(Ib.data_ptr()), 30, C.c_void_p(J.data_ptr()), 8,
                                   C.byref(C.c_void_p()), None)  # bad may be NULL
    assert st == F.SPL_ERROR_index_out_of_bounds
    # the same in four-byte indices
    I4, J4 = Ib.to(torch.int32), Jr.to(torch.int32)
    torch.cuda.synchronize()
    assert refused(20, I4, 30, J.to(torch.int32), 4) == (F.SPL_ERROR_index_out_of_bounds, 5)
    assert refused(20, I.to(torch.int32), 30, J4, 4) == (F.SPL_ERROR_invalid_matrix, -1)
    # a row block, after everything that is decided without the device
    t = base["real"]
    a, b = int(t.rp[1000]), int(t.rp[2002])
    blk = pkg.DeviceMatrix.from_csr(NR, NC, t.rp[1000:2003] - a, t.ci[a:b], t.v[a:b], row0=1000)
    assert raw_select(pkg, blk, 20, I, 30, J, 8)[:2] == (F.SPL_ERROR_argument_missing, None)
    assert raw_select(pkg, blk, 20, I, 30, J, 3)[:2] == (F.SPL_ERROR_argument_missing, None)
    assert raw_select(pkg, blk, NR - 1, None, 30, J, 8)[:2] == (F.SPL_ERROR_dimension_mismatch, None)
    with pytest.raises(F.SparseLinearError, match="first offending position: 5"):
        H.select(Ib, J)


# ---- 5. results are ordinary handles ----------------------------------------------------------------------------------

def spmv_reference_order(torch, H, x, y0):
    H.set_variant(1)  # the CSR-stream kernel: the reference's order of additions
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y0.copy()).cuda()
    H.spmv_dev(dx.data_ptr(), dy.data_ptr(), accumulate=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dy.cpu().numpy()


def test_results_multiply_like_the_sliced_matrix(gpu, O, base, handles):
    t, H = base["real"], handles["real"]
    rng = np.random.default_rng(17)
    # 4 000 rows and 3 000 columns in random order, the rows and columns of the salted entries among them
    special = np.flatnonzero(~np.isfinite(t.v))
    rows_in, cols_in = row_ids(t)[special], t.ci[special].astype(np.int64)
    p = rng.permutation(np.concatenate([rows_in, rng.permutation(np.setdiff1d(np.arange(NR), rows_in))[:4000 - len(rows_in)]]))
    q = rng.permutation(np.concatenate([cols_in, rng.permutation(np.setdiff1d(np.arange(NC), cols_in))[:3000 - len(cols_in)]]))
    for got, want in ((H.submatrix(1000, 5, 3501, 3995), np_window(t, 1000, 5, 3501, 3995)),
                      (H.select(p, q), np_select(t, p, q))):
        assert not np.all(np.isfinite(want.v))  # the salt is inside: inf, -inf and the NaN take part
        x, y0 = rng.standard_normal(want.ncols), rng.standard_normal(want.nrows)
        m = O.csr_to_csc_tuple(want.nrows, want.ncols, want.rp, want.ci, want.v)
        ref = O.axpy(m, x, y0)
        y = spmv_reference_order(gpu, got, x, y0)
        odd = np.flatnonzero(bits(y) != bits(ref))
        print("rows whose bits differ: %r; device %r, oracle %r" % (odd.tolist(), bits(y)[odd].tolist(), bits(ref)[odd].tolist()))
        assert same_bits(y, ref)


def test_lin_of_two_windows(gpu, O, base, handles):
    t, H = base["real"], handles["real"]
    w1, w2 = (1000, 5, 2500, 2000), (3400, 2050, 2500, 2000)
    a, b = np_window(t, *w1), np_window(t, *w2)
    want = O.lin(1.25, O.csr_to_csc_tuple(*a), -0.75, O.csr_to_csc_tuple(*b))
    got = H.submatrix(*w1).lin(1.25, H.submatrix(*w2), -0.75)
    cp, ri, v = export_csc_dev(gpu, got)
    assert np.array_equal(cp, want[2]) and np.array_equal(ri, want[3])
    odd = np.flatnonzero(bits(v) != bits(want[4]))
    print("entries whose bits differ: %r; device %r, oracle %r" % (odd.tolist(), bits(v)[odd].tolist(), bits(want[4])[odd].tolist()))
    assert same_bits(v, want[4])


def test_symmetric_permutation_stays_hermitian_and_solves(gpu, pkg):
    """select(p, p) of poisson2d(24): still Hermitian, and the LU from handles of it solves P A P^T y = P b with
    |y - P x|_inf <= 1e-10 |x|_inf (the contract of include/sparse_linear_hip.h) against the solution x of the
    unpermuted system by the same route"""
    torch = gpu
    U = pkg.umfpack
    A = pkg.DeviceMatrix.synthetic("poisson2d", 24)
    n = 24 * 24
    rng = np.random.default_rng(24)
    p = rng.permutation(n)
    PAPt = A.select(p, p)
    assert A.hermitian() and PAPt.hermitian()
    assert not A.select(p, rng.permutation(n)).hermitian()
    b = rng.standard_normal(n)

    def solve(H, rhs):
        f = U.factorDevice(H, U.analyzeDevice(H))
        B = torch.from_numpy(np.ascontiguousarray(rhs[None, :])).cuda()
        return U.linearSolveManyDevice_(f, U.UmfpackNormal, None, B).cpu().numpy()[0]

    x, y = solve(A, b), solve(PAPt, b[p])
    err, scale = float(np.max(np.abs(y - x[p]))), float(np.max(np.abs(x)))
    print("|y - P x|_inf = %.3g, |x|_inf = %.3g" % (err, scale))
    assert err <= 1e-10 * scale


# ---- 6. the Python surface ------------------------------------------------------------------------------------------

def test_getitem(gpu, base, handles):
    t, H = base["real"], handles["real"]
    assert_is(gpu, H[1000:2002, 5:4000], np_window(t, 1000, 5, 1002, 3995), csc=False)
    assert_is(gpu, H[:, 3003:], np_window(t, 0, 3003, NR, NC - 3003), csc=False)
    assert_is(gpu, H[-7:, :-99], np_window(t, NR - 7, 0, 7, NC - 99), csc=False)
    assert_is(gpu, H[5:3, :], np_window(t, 5, 0, 0, NC), csc=False)
    assert_is(gpu, H[[3, 3, 0], [2, 1]], np_select(t, [3, 3, 0], [2, 1]), csc=False)
    rows = gpu.tensor([LONG_ROW, 5, LONG_ROW], dtype=gpu.int32, device="cuda")
    cols = gpu.arange(NC - 1, -1, -1, dtype=gpu.int32, device="cuda")
    assert_is(gpu, H[rows, cols], np_select(t, [LONG_ROW, 5, LONG_ROW], np.arange(NC)[::-1]), csc=False)
    for key in ((slice(None, None, 2), slice(None)), (slice(0, 5), [1, 2]), 7, (1, 2)):
        with pytest.raises(TypeError):
            H[key]


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_host_subMatrix_agrees_with_numpy(gpu, pkg, base, kind):
    t = base[kind]
    cp, ri, v = np_csc(t)
    M = pkg.Matrix(NC, NR, cp, ri, v)
    for r0, c0, nr, nc in ((1000, 5, 1002, 3995), (0, 0, NR, NC), (LONG_ROW, 100, 1, 3000), (17, 23, 0, 5)):
        got = pkg.sparse.subMatrix((r0, c0), (nr, nc), M)
        want = np_csc(np_window(t, r0, c0, nr, nc))
        assert (got.nrows, got.ncols) == (nr, nc)
        assert np.array_equal(got.pointers, want[0]) and np.array_equal(got.indices, want[1])
        assert got.values.dtype == want[2].dtype and same_bits(got.values, want[2])
    for origin, shape, message in (((1, 0), (NR, 1), "range exceeds input row size"),
                                   ((0, 1), (1, NC), "range exceeds input column size")):
        with pytest.raises(pkg.SparseError, match=message):
            pkg.sparse.subMatrix(origin, shape, M)
