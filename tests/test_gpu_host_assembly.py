"""The host-tuple structural constructors spl_kronecker, spl_assemble_blocks (hcat, vcat, fromBlocks, fromBlocksDiag,
blockDiag) and spl_take_diag, through the Python functions and called raw.  They run the kernels of the device
handles on the caller's CSC arrays taken as the row image of the transpose, so what can go wrong here is that seam:
the exchange of rows and columns, the int32 -> int64 pointers, the column sort, the size checks made on the host.

Every expected value comes from the CPU oracle (O.kronecker, O.hcat, O.vcat, O.fromBlocks, O.fromBlocksDiag,
O.blockDiag, O.take_diag, O.zeros) or is written out in numpy; none from the handle route, which shares the code
under test.  Matrices are compared bit for bit: dimensions, pointers, indices, the bit patterns of the values."""
import ctypes as C

import numpy as np
import pytest

from helpers import mat_to_tuple, tuple_to_mat

pytestmark = pytest.mark.gpu

OK, INVALID, DIM, OVERFLOW = 0, -8, -20, -22
vp = C.c_void_p
CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])


# ---- construction and comparison ----------------------------------------------------------------------------------------

def values(rng, k, cplx=False):
    """rounding-order sensitive: a product formed another way shows in the last bits"""
    v = rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, k)
    return v + 1j * rng.standard_normal(k) if cplx else v


def from_mask(mask, vals):
    """CSC oracle tuple of a boolean pattern; vals in column-major order of the pattern"""
    cols, rows = np.nonzero(mask.T)
    p = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.int64)
    return (mask.shape[0], mask.shape[1], p, rows.astype(np.int64), np.asarray(vals))


def random_matrix(rng, nr, nc, k, cplx=False):
    mask = np.zeros(nr * nc, dtype=bool)
    mask[rng.choice(nr * nc, k, replace=False)] = True
    return from_mask(mask.reshape(nr, nc), values(rng, k, cplx))


def columns_of_length(rng, nr, nc, k):
    """every column holds exactly k entries"""
    mask = np.zeros((nr, nc), dtype=bool)
    for c in range(nc):
        mask[rng.choice(nr, k, replace=False), c] = True
    return from_mask(mask, values(rng, nc * k))


def reverse_columns(m):
    """the same matrix with the entries of every column in descending row order"""
    nr, nc, p, i, x = m
    i, x = i.copy(), x.copy()
    for c in range(nc):
        i[p[c]:p[c + 1]] = i[p[c]:p[c + 1]][::-1]
        x[p[c]:p[c + 1]] = x[p[c]:p[c + 1]][::-1]
    return (nr, nc, p, i, x)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def assert_same(got, want):
    assert (int(got[0]), int(got[1])) == (int(want[0]), int(want[1]))
    assert np.array_equal(np.asarray(got[2], dtype=np.int64), np.asarray(want[2], dtype=np.int64))
    assert np.array_equal(np.asarray(got[3], dtype=np.int64), np.asarray(want[3], dtype=np.int64))
    gv, wv = np.asarray(got[4]), np.asarray(want[4])
    if np.iscomplexobj(gv) or np.iscomplexobj(wv):
        gv, wv = gv.astype(np.complex128), wv.astype(np.complex128)
    assert np.array_equal(bits(gv), bits(wv))


@pytest.fixture(scope="module")
def L(pkg, gpu):
    return pkg._ffi.lib()


def c_tuple(m, keep):
    """an oracle tuple as the five ctypes arguments of the ABI; complex values as (re, im) pairs"""
    p, i = np.ascontiguousarray(m[2], dtype=np.int32), np.ascontiguousarray(m[3], dtype=np.int32)
    x = np.ascontiguousarray(m[4])
    x = x.view(np.float64) if np.iscomplexobj(x) else x.astype(np.float64)
    keep.append((p, i, x))
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    return (int(m[0]), int(m[1]), p.ctypes.data_as(ip), i.ctypes.data_as(ip), x.ctypes.data_as(dp))


def take_result(pkg, nrows, ncols, cp, ci, cx, cplx=False):
    p = pkg._ffi.take_malloced(cp, ncols + 1, C.c_int, np.int64)
    nz = int(p[-1])
    i = pkg._ffi.take_malloced(ci, max(nz, 1), C.c_int, np.int64)[:nz]
    x = pkg._ffi.take_malloced(cx, max(nz, 1) * (2 if cplx else 1), C.c_double, np.float64)[:nz * (2 if cplx else 1)]
    return (nrows, ncols, p, i, x.view(np.complex128) if cplx else x)


def kron_raw(pkg, L, a, b):
    """spl_kronecker on two oracle tuples: (status, result tuple or None); a refusal must leave every output NULL"""
    keep = []
    nr, nc, cp, ci, cx = C.c_int(-7), C.c_int(-7), vp(1), vp(1), vp(1)
    st = L.spl_kronecker(*c_tuple(a, keep), *c_tuple(b, keep), C.byref(nr), C.byref(nc), C.byref(cp), C.byref(ci),
                         C.byref(cx))
    if st != OK:
        assert not cp.value and not ci.value and not cx.value
        return st, None
    return st, take_result(pkg, nr.value, nc.value, cp, ci, cx)


def assemble_raw(pkg, L, blocks, row_off, col_off, nrows, ncols, cplx=False):
    """spl_assemble_blocks on oracle tuples listed as given: (status, result tuple or None)"""
    k, keep = len(blocks), []
    args = [c_tuple(m if not cplx else m[:4] + (np.asarray(m[4], dtype=np.complex128),), keep) for m in blocks]
    ints = lambda v: (C.c_int * max(k, 1))(*[int(t) for t in v])
    ptrs = lambda j: (vp * max(k, 1))(*[C.cast(t[j], vp) for t in args])
    cp, ci, cx = vp(1), vp(1), vp(1)
    fn = L.spl_assemble_blocks
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int,
                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    st = fn(k, ints([t[0] for t in args]), ints([t[1] for t in args]), ptrs(2), ptrs(3), ptrs(4), 2 if cplx else 1,
            ints(row_off), ints(col_off), nrows, ncols, C.byref(cp), C.byref(ci), C.byref(cx))
    if st != OK:
        assert not cp.value and not ci.value and not cx.value
        return st, None
    return st, take_result(pkg, nrows, ncols, cp, ci, cx, cplx)


def take_diag_raw(L, m):
    keep = []
    d = np.full(min(m[0], m[1]), np.nan)
    assert L.spl_take_diag(*c_tuple(m, keep), d.ctypes.data_as(C.POINTER(C.c_double))) == OK
    return d


# ---- spl_kronecker ------------------------------------------------------------------------------------------------------

def kron_both_ways(pkg, L, O, a, b):
    want = O.kronecker(a, b)
    assert_same(mat_to_tuple(pkg.kronecker(tuple_to_mat(pkg, a), tuple_to_mat(pkg, b))), want)
    st, got = kron_raw(pkg, L, a, b)
    assert st == OK
    assert_same(got, want)
    return want


def test_kronecker_rectangular_in_both_orders(gpu, pkg, L, O):
    rng = np.random.default_rng(597)
    a, b = random_matrix(rng, 2, 3, 4), random_matrix(rng, 5, 2, 7)
    assert (kron_both_ways(pkg, L, O, a, b)[:2]) == (10, 6)  # a swapped dimension shows as a wrong index
    assert (kron_both_ways(pkg, L, O, b, a)[:2]) == (10, 6)
    assert not np.array_equal(O.kronecker(a, b)[3], O.kronecker(b, a)[3])


def test_kronecker_empty_columns_1x1_and_no_entries(gpu, pkg, L, O):
    rng = np.random.default_rng(634)
    mask = np.zeros((7, 9), dtype=bool)
    mask[rng.choice(7, 4, replace=False), 1] = True
    mask[:, 4] = True
    mask[3, 8] = True  # columns 0, 2, 3, 5, 6, 7 are empty
    a = from_mask(mask, values(rng, int(mask.sum())))
    b = random_matrix(rng, 6, 5, 11)
    one = from_mask(np.ones((1, 1), dtype=bool), np.array([-2.5]))
    none = from_mask(np.zeros((3, 4), dtype=bool), np.zeros(0))
    for x, y in ((a, b), (b, a), (a, a), (a, one), (one, a), (one, one), (a, none), (none, a), (none, none)):
        kron_both_ways(pkg, L, O, x, y)


# column lengths (A, B): the mean result column length lenA * lenB makes the host choose 1, 4, 8, 8, 16, 32 lanes per
# column, and 64 for the two dense pairs (33 and 64 entries per column).  lenB = 3, 5, 7, 11 divide no lane count: the
# pair counters of the kernel wrap.  13 x 11 = 143 result columns are no multiple of what a workgroup takes.
KRON_REGIMES = [((6, 13), 1, (8, 11), 1), ((6, 13), 1, (8, 11), 3), ((6, 13), 1, (8, 11), 5), ((6, 13), 1, (8, 11), 7),
                ((6, 13), 2, (8, 11), 7), ((6, 13), 3, (8, 11), 7), ((3, 3), 3, (11, 11), 11), ((4, 4), 4, (16, 16), 16)]


@pytest.mark.parametrize("sa,ka,sb,kb", KRON_REGIMES, ids=["len%dx%d" % (r[1], r[3]) for r in KRON_REGIMES])
def test_kronecker_lane_group_regimes(gpu, pkg, L, O, sa, ka, sb, kb):
    rng = np.random.default_rng(100 * ka + kb)
    a, b = columns_of_length(rng, sa[0], sa[1], ka), columns_of_length(rng, sb[0], sb[1], kb)
    want = kron_both_ways(pkg, L, O, a, b)
    assert np.all(np.diff(want[2]) == ka * kb)


def test_kronecker_unsorted_columns_bitwise(gpu, pkg, L, O):
    rng = np.random.default_rng(401)
    a, b = random_matrix(rng, 6, 5, 17), random_matrix(rng, 4, 7, 15)
    st, got = kron_raw(pkg, L, reverse_columns(a), reverse_columns(b))
    assert st == OK
    assert_same(got, O.kronecker(a, b))


def test_kronecker_result_with_more_than_2_to_22_columns(gpu, pkg, L):
    """2049^2 = 4 198 401 result columns: the last 4 097 lie past what 2^20 workgroups of four columns reach, the grid
    limit a launch of one wavefront per column once had.  diag(a) (x) diag(b) = diag of the products b * a, in numpy."""
    m = 2049
    rng = np.random.default_rng(2049)
    a, b = values(rng, m), values(rng, m)
    diag = lambda v: (len(v), len(v), np.arange(len(v) + 1), np.arange(len(v)), v)
    st, got = kron_raw(pkg, L, diag(a), diag(b))
    assert st == OK
    assert_same(got, diag((a[:, None] * b[None, :]).ravel()))


def test_kronecker_entry_count_overflow_and_invalid_before_overflow(gpu, pkg, L):
    n = 216  # 216^2 = 46 656 rows, columns and entries: the dimensions of the product fit, 46 656^2 entries do not
    big = (n, n, np.arange(n + 1) * n, np.tile(np.arange(n), n), np.ones(n * n))
    assert kron_raw(pkg, L, big, big) == (OVERFLOW, None)
    bad = (3, 3, np.array([0, 3, 2, 5]), np.array([0, 2, 1, 0, 2]), np.ones(5))
    assert kron_raw(pkg, L, bad, big) == (INVALID, None)
    assert kron_raw(pkg, L, big, bad) == (INVALID, None)
    p = big[2].copy()
    p[100], p[101] = p[101], p[100]  # invalid and too large at once: the invalid tuple is reported
    assert kron_raw(pkg, L, big, (n, n, p, big[3], big[4])) == (INVALID, None)
    assert kron_raw(pkg, L, (n, n, p, big[3], big[4]), big) == (INVALID, None)


# ---- spl_assemble_blocks ------------------------------------------------------------------------------------------------

@CPLX
def test_vcat_and_hcat_of_three_with_empty_members(gpu, pkg, O, cplx):
    rng = np.random.default_rng(500)
    tall = [random_matrix(rng, 4, 6, 9, cplx), random_matrix(rng, 0, 6, 0, cplx), random_matrix(rng, 3, 6, 7, cplx)]
    wide = [random_matrix(rng, 5, 3, 6, cplx), random_matrix(rng, 5, 0, 0, cplx), random_matrix(rng, 5, 4, 8, cplx)]
    flat = [random_matrix(rng, h, 0, 0, cplx) for h in (2, 0, 3)]   # zero width, stacked
    thin = [random_matrix(rng, 0, w, 0, cplx) for w in (2, 0, 3)]   # zero height, side by side
    M = lambda ms: [tuple_to_mat(pkg, m) for m in ms]
    assert_same(mat_to_tuple(pkg.vcat(M(tall))), O.vcat(tall))
    assert_same(mat_to_tuple(pkg.hcat(M(wide))), O.hcat(wide))
    assert_same(mat_to_tuple(pkg.vcat(M(flat))), O.vcat(flat))
    assert_same(mat_to_tuple(pkg.hcat(M(thin))), O.hcat(thin))


@CPLX
def test_grid_with_holes_in_any_listing_order(gpu, pkg, L, O, cplx):
    rng = np.random.default_rng(563)
    heights, widths = [2, 3, 1, 4], [3, 1, 5]
    holes = {(0, 1), (1, 0), (2, 2), (3, 1)}
    grid = [[None if (r, c) in holes else random_matrix(rng, h, w, (h * w + 1) // 2, cplx) for c, w in enumerate(widths)]
            for r, h in enumerate(heights)]
    want = O.fromBlocks(grid)
    assert_same(mat_to_tuple(pkg.fromBlocks([[None if m is None else tuple_to_mat(pkg, m) for m in r] for r in grid])),
                want)
    roff, coff = np.concatenate([[0], np.cumsum(heights)]), np.concatenate([[0], np.cumsum(widths)])
    placed = [(grid[r][c], roff[r], coff[c]) for r in range(4) for c in range(3) if grid[r][c] is not None]
    for listing in (placed, placed[::-1]):
        st, got = assemble_raw(pkg, L, [t[0] for t in listing], [t[1] for t in listing], [t[2] for t in listing],
                               int(roff[-1]), int(coff[-1]), cplx)
        assert st == OK
        assert_same(got, want)


@CPLX
def test_block_diag_of_300_small_blocks(gpu, pkg, O, cplx):
    rng = np.random.default_rng(661)
    mats = []
    for b in range(300):
        h, w = 1 + b % 3, 1 + (b // 3) % 3
        mats.append(random_matrix(rng, h, w, int(rng.integers(0, h * w + 1)), cplx))
    assert_same(mat_to_tuple(pkg.blockDiag([tuple_to_mat(pkg, m) for m in mats])), O.blockDiag(mats))


def test_overlapping_blocks_are_refused(gpu, pkg, L):
    rng = np.random.default_rng(7)
    a, b = random_matrix(rng, 3, 3, 4), random_matrix(rng, 3, 3, 5)
    assert assemble_raw(pkg, L, [a, b], [0, 2], [0, 2], 5, 5) == (DIM, None)  # they share the cell (2, 2)
    assert assemble_raw(pkg, L, [b, a], [2, 0], [2, 0], 5, 5) == (DIM, None)
    assert assemble_raw(pkg, L, [a, b], [0, 3], [0, 2], 6, 5)[0] == OK       # rows apart: columns may be shared


def test_unsorted_block_keeps_its_order(gpu, pkg, L):
    # [[., 1], [2, .], [3, 4]] with its columns stored in the row orders (2, 1) and (2, 0), below the 1 x 2 block
    # [5, 6]: every result column is the upper block's entry, then the lower block's entries in the order they have
    low = (3, 2, np.array([0, 2, 4]), np.array([2, 1, 2, 0]), np.array([3.0, 2.0, 4.0, 1.0]))
    top = (1, 2, np.array([0, 1, 2]), np.array([0, 0]), np.array([5.0, 6.0]))
    want = (4, 2, np.array([0, 3, 6]), np.array([0, 3, 2, 0, 3, 1]), np.array([5.0, 3.0, 2.0, 6.0, 4.0, 1.0]))
    for blocks, ro in (([top, low], [0, 1]), ([low, top], [1, 0])):
        st, got = assemble_raw(pkg, L, blocks, ro, [0, 0], 4, 2)
        assert st == OK
        assert_same(got, want)


@pytest.mark.parametrize("shape", [(5, 7), (0, 7), (5, 0)])
def test_no_blocks_give_zeros(gpu, pkg, L, O, shape):
    st, got = assemble_raw(pkg, L, [], [], [], *shape)
    assert st == OK
    assert_same(got, O.zeros(*shape))


# ---- spl_take_diag ------------------------------------------------------------------------------------------------------

def test_take_diag(gpu, pkg, L, O):
    rng = np.random.default_rng(640)
    dense = from_mask(np.ones((20, 20), dtype=bool), values(rng, 400))  # a column longer than the 8 searching lanes
    wide, tall = random_matrix(rng, 3, 7, 12), random_matrix(rng, 7, 3, 12)
    none = from_mask(np.zeros((4, 6), dtype=bool), np.zeros(0))
    mask = np.zeros((5, 5), dtype=bool)
    mask[[0, 2, 4, 2, 3, 4], [0, 0, 1, 2, 2, 4]] = True
    zero = from_mask(mask, np.array([0.0, 7.0, 1.5, -0.0, 3.0, 2.0]))  # stored zeros at (0, 0) and (2, 2), (3, 3) absent
    assert zero[3][3] == 2 and np.signbit(zero[4][3])
    for m in (wide, tall, dense, none, zero):
        want = O.take_diag(m)
        assert len(want) == min(m[0], m[1])
        assert np.array_equal(bits(take_diag_raw(L, m)), bits(want))
        assert np.array_equal(bits(pkg.takeDiag(tuple_to_mat(pkg, m))), bits(want))
    for m in (wide, tall, dense, zero):
        assert np.array_equal(bits(take_diag_raw(L, reverse_columns(m))), bits(O.take_diag(m)))  # unsorted columns
