"""The structural constructors on device handles: spl_matrix_kronecker, spl_matrix_assemble_blocks (hcat, vcat,
fromBlocks, fromBlocksDiag, blockDiag), spl_matrix_take_diag_dev and spl_matrix_diag_dev / ident, and what they make
fed back into the rest of the handle family.

Every expected value comes from the CPU oracle (O.kronecker, O.fromBlocks, O.hcat, O.vcat, O.fromBlocksDiag,
O.blockDiag, O.take_diag, O.lin, O.transpose, O.mulV) or from plain numpy; none from the library under test.  Every
comparison of a matrix is bit for bit: dimensions, pointers, indices and the bit patterns of the values.

A full row and an empty column cannot live in one matrix, so the Kronecker operands come in two copies of one
pattern: `full` (rows of length 0, 1 and ncols) and `gap` (the same with one column emptied)."""
import numpy as np
import pytest

from helpers import handle_to_csc_tuple

pytestmark = pytest.mark.gpu

ARG, DIM = -5, -20  # SPL_ERROR_argument_missing, SPL_ERROR_dimension_mismatch


# ---- host-side construction -------------------------------------------------------------------------------------------

def values(rng, k, cplx=False):
    """rounding-order sensitive: a product or sum formed another way shows in the last bits"""
    v = rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, k)
    if not cplx:
        return v
    w = rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, k)
    z = v + 1j * w
    if k >= 6:  # a zero real part, a zero imaginary part: a wrong sign or a swapped addend shows
        z[1::6] = 1j * w[1::6]
        z[4::6] = v[4::6] + 0j
    return z


def from_mask(mask, vals):
    """CSC oracle tuple of a boolean pattern; vals in column-major order of the pattern"""
    nr, nc = mask.shape
    cols, rows = np.nonzero(mask.T)  # column by column, rows ascending
    p = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.int64)
    assert len(vals) == len(rows)
    return (nr, nc, p, rows.astype(np.int64), np.asarray(vals))


def random_mask(rng, nr, nc, k):
    mask = np.zeros(nr * nc, dtype=bool)
    mask[rng.choice(nr * nc, k, replace=False)] = True
    return mask.reshape(nr, nc)


def rows_of_length(rng, nr, nc, k):
    """every row holds exactly k entries"""
    mask = np.zeros((nr, nc), dtype=bool)
    for r in range(nr):
        mask[r, rng.choice(nc, k, replace=False)] = True
    return mask


def operand_masks(rng, nr, nc, k):
    """`full`: row 0 empty, row 1 one entry, row 2 full; `gap`: the same pattern with column 3 emptied"""
    mask = random_mask(rng, nr, nc, k)
    mask[0, :] = False
    mask[1, :] = False
    mask[1, nc // 2] = True
    mask[2, :] = True
    gap = mask.copy()
    gap[:, 3] = False
    return mask, gap


def parts(m):
    return (m[0], m[1], m[2], m[3], np.ascontiguousarray(m[4].real)), (m[0], m[1], m[2], m[3], np.ascontiguousarray(m[4].imag))


def kron_z(O, a, b):
    """A (x) B on Complex Double from four real oracle products: b * a = (br*ar - bi*ai) :+ (br*ai + bi*ar), the
    real operations numpy's (separately rounded); numpy's own complex multiply may fuse and is not used"""
    ar, ai = parts(a)
    br, bi = parts(b)
    rr, ii = O.kronecker(ar, br), O.kronecker(ai, bi)      # br*ar, bi*ai
    ri, ir = O.kronecker(ai, br), O.kronecker(ar, bi)      # br*ai, bi*ar
    re = rr[4] - ii[4]
    im = ri[4] + ir[4]
    z = np.empty(len(re), dtype=np.complex128)
    z.real, z.imag = re, im
    return (rr[0], rr[1], rr[2], rr[3], z)


def handle(pkg, m):
    M = pkg.Matrix(m[1], m[0], m[2], m[3], m[4])
    return pkg.DeviceMatrix.from_csc_complex(M) if M.is_complex else pkg.DeviceMatrix.from_csc(M)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def assert_same(H, want, cplx=None):
    """the handle's matrix against an oracle tuple, bit for bit"""
    got = handle_to_csc_tuple(H)
    inf = H.info()
    assert inf["row0"] == 0 and inf["nrows_local"] == inf["nrows_global"]
    assert (got[0], got[1]) == (int(want[0]), int(want[1])), ((got[0], got[1]), (want[0], want[1]))
    assert inf["nnz"] == len(want[3])
    assert np.array_equal(got[2], np.asarray(want[2], dtype=np.int64))
    assert np.array_equal(got[3], np.asarray(want[3], dtype=np.int64))
    wv = np.asarray(want[4])
    if cplx is None:
        cplx = np.iscomplexobj(wv)
    assert H.is_complex == bool(cplx)
    wv = wv.astype(np.complex128) if cplx else wv.astype(np.float64)
    assert got[4].dtype == wv.dtype
    assert np.array_equal(bits(got[4]), bits(wv))


def row_lengths(m):
    return np.bincount(np.asarray(m[3], dtype=np.int64), minlength=m[0])


def status_of(pkg, call):
    with pytest.raises(pkg._ffi.SparseLinearError) as e:
        call()
    return e.value.status


# ---- kronecker ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def operands():
    """A 37 x 29 and B 23 x 41, about 150 and 200 entries, real and complex on the same patterns"""
    rng = np.random.default_rng(597_634)
    out = {}
    for name, (nr, nc, k) in {"A": (37, 29, 130), "B": (23, 41, 170)}.items():
        full, gap = operand_masks(rng, nr, nc, k)
        for kind, mask in (("full", full), ("gap", gap)):
            n = int(mask.sum())
            out[name, kind, False] = from_mask(mask, values(rng, n))
            out[name, kind, True] = from_mask(mask, values(rng, n, True))
            lens = mask.sum(axis=1)
            assert lens[0] == 0 and lens[1] == 1
            assert (lens[2] == nc) == (kind == "full") and (mask.sum(axis=0).min() == 0) == (kind == "gap")
    return out


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("kind", ["full", "gap"])
def test_kronecker_both_orders(gpu, pkg, O, operands, kind, cplx):
    a, b = operands["A", kind, cplx], operands["B", kind, cplx]
    kron = (lambda x, y: kron_z(O, x, y)) if cplx else O.kronecker
    Ha, Hb = handle(pkg, a), handle(pkg, b)
    want = kron(a, b)
    if kind == "full":
        assert row_lengths(want).max() == 29 * 41  # the longest product row: 1189 entries
    assert_same(Ha.kronecker(Hb), want)
    assert_same(Hb.kronecker(Ha), kron(b, a))  # (x) is not commutative


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_kronecker_with_a_1x1_operand_and_with_an_operand_without_entries(gpu, pkg, O, operands, cplx):
    a = operands["A", "full", cplx]
    kron = (lambda x, y: kron_z(O, x, y)) if cplx else O.kronecker
    one = from_mask(np.ones((1, 1), dtype=bool), np.array([-2.5 + 0.75j]) if cplx else np.array([-2.5]))
    none = from_mask(np.zeros((3, 4), dtype=bool), np.zeros(0, dtype=np.complex128 if cplx else np.float64))
    Ha, H1, H0 = handle(pkg, a), handle(pkg, one), handle(pkg, none)
    assert_same(Ha.kronecker(H1), kron(a, one))
    assert_same(H1.kronecker(Ha), kron(one, a))
    assert_same(Ha.kronecker(H0), kron(a, none), cplx)
    assert_same(H0.kronecker(Ha), kron(none, a), cplx)
    assert_same(H0.kronecker(H0), kron(none, none), cplx)


def test_kronecker_refuses_a_real_with_a_complex_operand(gpu, pkg, operands):
    import ctypes as C
    Hr, Hz = handle(pkg, operands["A", "gap", False]), handle(pkg, operands["B", "gap", True])
    L = pkg._ffi.lib()
    for x, y in ((Hr, Hz), (Hz, Hr)):
        h = C.c_void_p(0x1234)
        assert L.spl_matrix_kronecker(x.handle, y.handle, C.byref(h)) == ARG and not h.value


# mean product row length -> lanes per row the host picks: 1 -> 1, 2 -> 2, 3 -> 4, 6 -> 8, 9 -> 16, 24 -> 32, 40 and
# 81 -> 64.  13 x 11 = 143 result rows: no multiple of the 256, 128, 64, 32, 16, 8 or 4 rows a workgroup takes.
REGIMES = [(1, 1), (1, 2), (1, 3), (2, 3), (3, 3), (3, 8), (5, 8), (9, 9)]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("ka,kb", REGIMES, ids=["mean%d" % (a * b) for a, b in REGIMES])
def test_kronecker_lane_group_regimes(gpu, pkg, O, ka, kb, cplx):
    rng = np.random.default_rng(1000 * ka + kb)
    ma, mb = rows_of_length(rng, 13, 12, ka), rows_of_length(rng, 11, 10, kb)
    a, b = from_mask(ma, values(rng, 13 * ka, cplx)), from_mask(mb, values(rng, 11 * kb, cplx))
    kron = (lambda x, y: kron_z(O, x, y)) if cplx else O.kronecker
    want = kron(a, b)
    assert len(want[3]) == 143 * ka * kb
    assert_same(handle(pkg, a).kronecker(handle(pkg, b)), want)


# ---- the model problem, end to end --------------------------------------------------------------------------------------

M_ORDER = 33


@pytest.fixture(scope="module")
def laplacian(O):
    m = M_ORDER
    mask = np.zeros((m, m), dtype=bool)
    i = np.arange(m)
    mask[i, i] = True
    mask[i[:-1], i[:-1] + 1] = True
    mask[i[:-1] + 1, i[:-1]] = True
    T = from_mask(mask, np.where(np.nonzero(mask.T)[0] == np.nonzero(mask.T)[1], 2.0, -1.0))
    I = (m, m, np.arange(m + 1, dtype=np.int64), np.arange(m, dtype=np.int64), np.ones(m))
    return T, I, O.lin(1.0, O.kronecker(I, T), 1.0, O.kronecker(T, I))


def device_laplacian(pkg, T):
    HT, HI = handle(pkg, T), pkg.DeviceMatrix.ident(M_ORDER)
    return HI.kronecker(HT).lin(1, HT.kronecker(HI), 1)


def test_model_problem_assembled_factored_and_solved_on_the_device(gpu, pkg, O, laplacian):
    import scipy.sparse as sp
    T, I, want = laplacian
    assert_same(pkg.DeviceMatrix.ident(M_ORDER), I)
    H = device_laplacian(pkg, T)
    assert_same(H, want)
    U = pkg.umfpack
    fd = U.factorDevice(H, U.analyzeDevice(H))
    n = M_ORDER * M_ORDER
    rng = np.random.default_rng(7)
    B = gpu.from_numpy(rng.normal(size=(3, n))).cuda()
    X = U.linearSolveManyDevice_(fd, U.UmfpackNormal, None, B).cpu().numpy()
    S = sp.csc_matrix((want[4], want[3], want[2]), shape=(n, n))
    Bh = B.cpu().numpy()
    for c in range(3):
        r = np.abs(S @ X[c] - Bh[c])
        den = abs(S) @ np.abs(X[c]) + np.abs(Bh[c])
        err = float(np.max(r / np.where(den > 0, den, 1.0)))
        print("componentwise backward error, column %d: %.3g" % (c, err))
        assert err <= 1e-13


# ---- block assembly -----------------------------------------------------------------------------------------------------

HEIGHTS, WIDTHS = (5, 0, 70), (4, 3, 70)


def grid_blocks(cplx):
    """the 3 x 3 grid: None at (0,1), (1,0), (1,2); block row 1 has no rows and holds a single block; block (2,2) has
    a row of 70 entries; block row 2 has rows made of three blocks; result rows 4 and 5 (either side of the boundary
    between block rows 0 and 2) are empty"""
    rng = np.random.default_rng(500_595)
    grid = [[None] * 3 for _ in range(3)]
    for r, c, k in ((0, 0, 8), (0, 2, 60), (1, 1, 0), (2, 0, 90), (2, 1, 70), (2, 2, 600)):
        h, w = HEIGHTS[r], WIDTHS[c]
        mask = random_mask(rng, h, w, k) if h * w else np.zeros((h, w), dtype=bool)
        if r == 0:
            mask[4, :] = False
        if r == 2:
            mask[0, :] = False
            mask[11, :] = True   # a row of 4 + 3 + 70 entries, 70 of them inside one block
            mask[12, 0] = True   # every block contributes to row 12 as well
        grid[r][c] = from_mask(mask, values(rng, int(mask.sum()), cplx))
    return grid


def placed(grid):
    ro, co = np.concatenate([[0], np.cumsum(HEIGHTS)]), np.concatenate([[0], np.cumsum(WIDTHS)])
    return [(grid[r][c], int(ro[r]), int(co[c])) for r in range(3) for c in range(3) if grid[r][c] is not None]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_from_blocks_grid_with_holes_in_either_listing_order(gpu, pkg, O, cplx):
    grid = grid_blocks(cplx)
    want = O.fromBlocks(grid)
    assert (want[0], want[1]) == (75, 77)
    lens = row_lengths(want)
    assert lens[4] == 0 and lens[5] == 0 and lens[5 + 11] == 77
    DM = pkg.DeviceMatrix
    hs = [[None if m is None else handle(pkg, m) for m in row] for row in grid]
    assert_same(DM.from_blocks(hs), want, cplx)
    pl = placed(hs)
    for order in (pl, pl[::-1]):
        assert_same(DM.assemble([p[0] for p in order], [p[1] for p in order], [p[2] for p in order], 75, 77), want, cplx)


def test_from_blocks_keeps_the_messages_of_the_host_function(gpu, pkg, O):
    DM = pkg.DeviceMatrix
    rng = np.random.default_rng(3)
    a = handle(pkg, from_mask(random_mask(rng, 3, 4, 5), values(rng, 5)))
    b = handle(pkg, from_mask(random_mask(rng, 2, 4, 3), values(rng, 3)))
    for grid, message in (([[a, None], [None, None]], "fromBlocks: underspecified heights"),
                          ([[a, b]], "fromBlocks: incompatible heights"),
                          ([[a, None], [b, None]], "fromBlocks: underspecified widths")):
        with pytest.raises(pkg.SparseError) as e:
            DM.from_blocks(grid)
        assert str(e.value) == message


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_hcat_and_vcat_of_three(gpu, pkg, O, cplx):
    rng = np.random.default_rng(504_559)
    DM = pkg.DeviceMatrix
    wide = [from_mask(random_mask(rng, 9, w, k), values(rng, k, cplx)) for w, k in ((5, 14), (1, 3), (7, 30))]
    assert_same(DM.hcat([handle(pkg, m) for m in wide]), O.hcat(wide), cplx)
    tall = [from_mask(random_mask(rng, h, 6, k), values(rng, k, cplx)) for h, k in ((4, 9), (1, 2), (8, 25))]
    assert_same(DM.vcat([handle(pkg, m) for m in tall]), O.vcat(tall), cplx)
    with pytest.raises(pkg.SparseError):
        DM.hcat([handle(pkg, wide[0]), handle(pkg, tall[0])])
    with pytest.raises(pkg.SparseError):
        DM.vcat([handle(pkg, wide[0]), handle(pkg, tall[0])])


def test_from_blocks_diag_with_two_super_diagonals(gpu, pkg, O):
    rng = np.random.default_rng(589_597)
    hs_, ws_ = (6, 3, 9), (5, 8, 4)

    def blk(r, c):
        k = hs_[r] * ws_[c] // 3
        return from_mask(random_mask(rng, hs_[r], ws_[c], k), values(rng, k))

    diags = [[blk(0, 0), blk(1, 1), blk(2, 2)], [blk(0, 1), blk(1, 2)], [blk(0, 2)]]
    want = O.fromBlocksDiag(diags)
    assert (want[0], want[1]) == (18, 17)
    assert_same(pkg.DeviceMatrix.from_blocks_diag([[handle(pkg, m) for m in d] for d in diags]), want)


def test_block_diag_of_300_small_blocks(gpu, pkg, O):
    rng = np.random.default_rng(661_667)
    mats = []
    for _ in range(300):
        h, w = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        k = int(rng.integers(0, h * w + 1))
        mats.append(from_mask(random_mask(rng, h, w, k) if h * w else np.zeros((h, w), dtype=bool), values(rng, k)))
    want = O.blockDiag(mats)
    assert_same(pkg.DeviceMatrix.block_diag([handle(pkg, m) for m in mats]), want)


def test_assemble_refuses_overlaps_and_blocks_that_leave_the_result(gpu, pkg, O):
    rng = np.random.default_rng(11)
    DM = pkg.DeviceMatrix
    ma, mb = from_mask(random_mask(rng, 3, 3, 4), values(rng, 4)), from_mask(random_mask(rng, 3, 3, 5), values(rng, 5))
    a, b = handle(pkg, ma), handle(pkg, mb)
    z = handle(pkg, from_mask(random_mask(rng, 3, 3, 5), values(rng, 5, True)))
    assert status_of(pkg, lambda: DM.assemble([a, b], [0, 2], [0, 2], 6, 6)) == DIM       # they share entry (2, 2)
    assert status_of(pkg, lambda: DM.assemble([b, a], [2, 0], [2, 0], 6, 6)) == DIM
    assert status_of(pkg, lambda: DM.assemble([a, b], [0, 0], [0, 0], 6, 6)) == DIM
    assert status_of(pkg, lambda: DM.assemble([a, b], [0, 4], [0, 3], 6, 6)) == DIM       # rows 4 .. 6 of 6
    assert status_of(pkg, lambda: DM.assemble([a, b], [0, 3], [0, 4], 6, 6)) == DIM       # columns 4 .. 6 of 6
    assert status_of(pkg, lambda: DM.assemble([a], [-1], [0], 6, 6)) == DIM
    assert status_of(pkg, lambda: DM.assemble([a, z], [0, 3], [0, 3], 6, 6)) == ARG       # a real with a complex block
    # touching rectangles are disjoint
    want = O.fromBlocks([[ma, None], [None, mb]])
    assert_same(DM.assemble([b, a], [3, 0], [3, 0], 6, 6), want)
    assert_same(DM.assemble([], [], [], 5, 7), O.zeros(5, 7))
    assert_same(DM.assemble([], [], [], 0, 7), O.zeros(0, 7))
    assert_same(DM.assemble([], [], [], 5, 0), O.zeros(5, 0))


# ---- diagonals ----------------------------------------------------------------------------------------------------------

def diag_case(rng, nr, nc, cplx):
    """some diagonal entries stored, some missing, one a stored zero; a row (45 x 70) or a column (70 x 45) of 70"""
    mask = random_mask(rng, nr, nc, nr * nc // 10)
    n = min(nr, nc)
    d = np.arange(n)
    mask[d, d] = rng.random(n) < 0.5
    mask[6, 6] = True    # the stored zero
    mask[9, 9] = False
    if nc > nr:
        mask[10, :] = True
    else:
        mask[:, 10] = True
    cols, rows = np.nonzero(mask.T)
    v = values(rng, len(rows), cplx)
    v[(rows == 6) & (cols == 6)] = 0.0
    return from_mask(mask, v)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("shape", [(70, 45), (45, 70)], ids=["70x45", "45x70"])
def test_take_diag(gpu, pkg, O, shape, cplx):
    m = diag_case(np.random.default_rng(640_650), shape[0], shape[1], cplx)
    if cplx:
        re, im = parts(m)
        want = np.empty(45, dtype=np.complex128)
        want.real, want.imag = O.take_diag(re), O.take_diag(im)
    else:
        want = O.take_diag(m)
    assert np.count_nonzero(want) not in (0, 45) and want[6] == 0 and want[10] != 0
    got = handle(pkg, m).take_diag()
    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_diag_dev_round_trips_through_take_diag(gpu, pkg, O, cplx):
    n = 1000  # four workgroups of the kernel, the last one partly filled
    d = values(np.random.default_rng(652_659), n, cplx)
    dd = gpu.from_numpy(d).cuda()
    H = pkg.DeviceMatrix.diag_dev(n, dd.data_ptr(), complex=cplx)
    assert_same(H, (n, n, np.arange(n + 1), np.arange(n), d), cplx)
    got = H.take_diag()
    assert np.array_equal(bits(got), bits(d))
    assert_same(pkg.DeviceMatrix.ident(n, complex=cplx), (n, n, np.arange(n + 1), np.arange(n), np.ones(n)), cplx)


def test_ident_times_a_matrix_is_the_matrix(gpu, pkg, O, operands):
    a = operands["A", "full", False]
    C_, products = pkg.DeviceMatrix.ident(37).spgemm(handle(pkg, a))
    assert products == len(a[3])
    assert_same(C_, a)


def test_diag_dev_of_nothing(gpu, pkg, O):
    for cplx in (False, True):
        H = pkg.DeviceMatrix.diag_dev(0, complex=cplx)
        assert_same(H, O.zeros(0, 0), cplx)
        assert len(H.take_diag()) == 0


# ---- what they make goes through the rest of the family -------------------------------------------------------------------

def spmv(torch, O, H, want_csc):
    nr, nc = want_csc[0], want_csc[1]
    xh = O.gen_vector(nc)
    x = torch.from_numpy(xh).cuda()
    y = torch.zeros(nr, dtype=torch.float64, device="cuda")
    assert H.spmv_kernel() == 0  # the CSR-stream kernel: reference order on rows within one chunk
    H.spmv_dev(x.data_ptr(), y.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu().numpy(), O.mulV(want_csc, xh)


def test_assembled_laplacian_through_spmv_transpose_hermitian_export(gpu, pkg, O, laplacian):
    T, I, want = laplacian
    H = device_laplacian(pkg, T)
    y, yo = spmv(gpu, O, H, want)
    assert np.array_equal(y, yo)
    assert H.hermitian() is True
    assert H.to_complex().hermitian() is True
    assert_same(H.transpose(), O.transpose(want))
    cp, ri, v = H.export_csc()
    assert np.array_equal(cp, want[2]) and np.array_equal(ri, want[3]) and np.array_equal(bits(v), bits(want[4]))


def test_assembled_grid_and_product_through_spmv_transpose_hermitian_export(gpu, pkg, O, operands):
    grid = grid_blocks(False)
    want = O.fromBlocks(grid)
    H = pkg.DeviceMatrix.from_blocks([[None if m is None else handle(pkg, m) for m in row] for row in grid])
    y, yo = spmv(gpu, O, H, want)
    assert np.array_equal(y, yo)
    assert H.hermitian() is False
    assert_same(H.transpose(), O.transpose(want))
    cp, ri, v = H.export_csc()
    assert np.array_equal(cp, want[2]) and np.array_equal(ri, want[3]) and np.array_equal(bits(v), bits(want[4]))
    # a product of products: (A (x) B)^T, and a lin on top of two Kronecker products of one shape
    a, b = operands["A", "gap", False], operands["B", "gap", False]
    K = handle(pkg, a).kronecker(handle(pkg, b))
    wantK = O.kronecker(a, b)
    assert_same(K.transpose(), O.kronecker(O.transpose(a), O.transpose(b)))  # (A (x) B)^T = A^T (x) B^T
    assert_same(K.lin(1.5, K, -0.25), O.lin(1.5, wantK, -0.25, wantK))
    d = K.take_diag()
    assert np.array_equal(bits(d), bits(O.take_diag(wantK)))
