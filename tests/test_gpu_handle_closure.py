"""The device-resident handle family of include/sparse_linear_hip.h composed with itself and with row blocks:
every way to obtain a handle (from_csc whole and nnz-balanced parts, from_csr whole and row blocks, compress_dev,
lin, spgemm, transpose, to_complex — the binary ones on row blocks too), each export (export_csr, export_csr_rows
with its capacity protocol, export_csc with local row ids), derived handles consumed again (SpMV on the stream
kernel and on every image, SpMM, a second lin / spgemm on top of results), the refusals the header states, CSR
input with unsorted rows, and reserved CUs.

Every expected value comes from the CPU oracle (O.compress, O.transpose, O.lin, O.lin_z, O.mm, O.mulV_z, O.axpy,
O.axpy_z, O.csr_gaxpy32, O.gen_random_csr) or from numpy slicing of oracle output; none from the library under
test.  One rectangular base matrix (6 007 x 4 099, about 60 000 entries, empty rows at both ends and at the cut
2 002, one row of 300 entries — below the stream kernel's 512-entry chunk, so its bit-identity claim holds) in two
copies: generic doubles, and small integers for the order-free checks.  Reference-order kernels are compared bit
for bit; the order-free panel image with the contract of tests/test_gpu_spmv_panel_rounds.py (1e-10 closeness,
2 len eps sum |a x| per row, bit equality on integer data, panel_errors() == 0)."""
import collections
import ctypes as C

import numpy as np
import pytest

from helpers import handle_to_csc_tuple

pytestmark = pytest.mark.gpu

NR, NC, NCB = 6007, 4099, 3001          # A, A2: NR x NC; B: NC x NCB
EMPTY_ROWS = (0, 2001, 2002, 2003, NR - 1)
LONG_ROW, LONG_LEN = 3000, 300
# cuts that are no multiple of 64, heights that are no multiple of 256; empty rows on both sides of the cut 2002
BLOCKS = {"blk0": (0, 1000), "blk1": (1000, 2002), "blk2": (2002, 4501), "blk3": (4501, NR),
          "zero": (2002, 2002), "one": (LONG_ROW, LONG_ROW + 1), "empty": (2001, 2004)}
ALPHA, BETA = 1.25, -0.75               # exact on the integer copy as well
ARG = -5  # SPL_ERROR_argument_missing
EPS = np.finfo(float).eps

# rows [row0, row0 + len(rp) - 1) of an nrows_global x ncols matrix as CSR arrays relative to the block
Truth = collections.namedtuple("Truth", "nrows_global ncols row0 rp ci v")


def nloc(t):
    return len(t.rp) - 1


def rows_of(t, r0, r1):
    """rows [r0, r1) (local numbering) of a truth, as a truth"""
    a, b = int(t.rp[r0]), int(t.rp[r1])
    return Truth(t.nrows_global, t.ncols, t.row0 + r0, t.rp[r0:r1 + 1] - a, t.ci[a:b], t.v[a:b])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def as_csc(O, t):
    """the CSC oracle tuple (local row ids) of a truth"""
    return O.transpose((t.ncols, nloc(t), t.rp, t.ci, t.v))


class Data(object):
    """host side of one copy (generic or integer values) of the base matrices, oracle results cached"""

    def __init__(self, O, integer):
        self.O = O
        rng = np.random.default_rng(20_24)

        def values(k):
            if integer:
                return rng.integers(-9, 10, k).astype(float)
            return rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, k)  # rounding-order sensitive

        def pattern(nr, nc, k, forbidden_rows=()):
            key = np.unique(rng.integers(0, nr, k) * nc + rng.integers(0, nc, k))  # no duplicates
            r, c = key // nc, key % nc
            keep = ~np.isin(r, forbidden_rows)
            return r[keep], c[keep]

        r, c = pattern(NR, NC, 60_500, EMPTY_ROWS + (LONG_ROW,))
        r = np.concatenate([r, np.full(LONG_LEN, LONG_ROW)])
        c = np.concatenate([c, rng.choice(NC, LONG_LEN, replace=False)])
        order = rng.permutation(len(r))  # the triples in no particular order
        self.triples = (r[order].astype(np.int32), c[order].astype(np.int32), values(len(r)))
        self.A = O.compress(NR, NC, *self.triples)
        # A2: half of A's positions and as many others, so lin meets shared and one-sided entries
        r2, c2 = pattern(NR, NC, 30_000, EMPTY_ROWS + (LONG_ROW,))
        half = rng.permutation(len(r))[: len(r) // 2]
        key2 = np.unique(np.concatenate([r[half] * NC + c[half], r2 * NC + c2]))
        self.A2 = O.compress(NR, NC, key2 // NC, key2 % NC, values(len(key2)))
        rb, cb = pattern(NC, NCB, 40_000)
        self.B = O.compress(NC, NCB, rb, cb, values(len(rb)))
        self._cache = {}

    def csr(self, csc):
        t = self.O.transpose(csc)  # the CSC arrays of the transpose are the CSR arrays
        return Truth(csc[0], csc[1], 0, t[2], t[3], t[4])

    def get(self, name):
        if name not in self._cache:
            O = self.O
            make = {
                "A": lambda: self.csr(self.A),
                "A2": lambda: self.csr(self.A2),
                "B": lambda: self.csr(self.B),
                "lin": lambda: self.csr(self.get("lin_csc")),
                "lin_csc": lambda: O.lin(ALPHA, self.A, BETA, self.A2),
                "AB_csc": lambda: O.mm(self.A, self.B),
                "A2B_csc": lambda: O.mm(self.A2, self.B),
                "AB": lambda: self.csr(self.get("AB_csc")),
                "At": lambda: Truth(NC, NR, 0, self.A[2], self.A[3], self.A[4]),
                # second generation: alpha (A B) + beta (A2 B), and (alpha A + beta A2) A^T
                "lin_of_products": lambda: self.csr(O.lin(ALPHA, self.get("AB_csc"), BETA, self.get("A2B_csc"))),
                "product_of_lin": lambda: self.csr(O.mm(self.get("lin_csc"), O.transpose(self.A))),
            }
            self._cache[name] = make[name]()
        return self._cache[name]


@pytest.fixture(scope="module")
def data(O):
    return {"generic": Data(O, False), "integer": Data(O, True)}


@pytest.fixture(scope="module")
def L(pkg, gpu):
    return pkg._ffi.lib()


# ---- producers: name -> (handle, truth) --------------------------------------------------------------------------

def csr_handle(pkg, t):
    return pkg.DeviceMatrix.from_csr(t.nrows_global, t.ncols, t.rp, t.ci, t.v, row0=t.row0)


def csc_handle(pkg, csc, part=0, nparts=1):
    return pkg.DeviceMatrix.from_csc(pkg.Matrix(csc[1], csc[0], csc[2], csc[3], csc[4]), part=part, nparts=nparts)


def part_bounds(rp, p, nparts):
    """the rule of spl_matrix_create_rowblock: block p starts at the first row whose pointer is >= nnz * p / nparts"""
    nnz, nrows = int(rp[-1]), len(rp) - 1
    cut = [0 if q <= 0 else nrows if q >= nparts else int(np.searchsorted(rp, (nnz * q) // nparts, side="left"))
           for q in (p, p + 1)]
    return cut[0], cut[1]


def block(d, which, blk):
    t = d.get(which)
    return rows_of(t, *BLOCKS[blk])


def produce(torch, pkg, d, name):
    """a fresh handle made the way `name` says, and the truth it has to hold"""
    kind, _, arg = name.partition(":")
    A = d.get("A")
    if kind == "csc":
        if arg == "whole":
            return csc_handle(pkg, d.A), A
        p = int(arg)
        return csc_handle(pkg, d.A, p, 3), rows_of(A, *part_bounds(A.rp, p, 3))
    if kind == "csr":
        t = A if arg == "whole" else block(d, "A", arg)
        return csr_handle(pkg, t), t
    if kind == "compress_dev":
        r, c, v = (torch.from_numpy(a).cuda() for a in d.triples)
        return pkg.DeviceMatrix.compress_dev(NR, NC, len(d.triples[0]), r.data_ptr(), c.data_ptr(), v.data_ptr()), A
    if kind == "lin":
        if arg == "whole":
            return csc_handle(pkg, d.A).lin(ALPHA, csc_handle(pkg, d.A2), BETA), d.get("lin")
        HA, HB = csr_handle(pkg, block(d, "A", arg)), csr_handle(pkg, block(d, "A2", arg))
        return HA.lin(ALPHA, HB, BETA), block(d, "lin", arg)
    if kind == "spgemm":
        HB = csc_handle(pkg, d.B)
        if arg == "whole":
            return csc_handle(pkg, d.A).spgemm(HB)[0], d.get("AB")
        return csr_handle(pkg, block(d, "A", arg)).spgemm(HB)[0], block(d, "AB", arg)
    if kind == "transpose":
        return csc_handle(pkg, d.A).transpose(), d.get("At")
    if kind == "to_complex":
        t = A if arg == "whole" else block(d, "A", arg)
        return csr_handle(pkg, t).to_complex(), t._replace(v=t.v + 0j)
    raise KeyError(name)


PRODUCERS = (["csc:whole", "csc:0", "csc:1", "csc:2", "csr:whole"] + ["csr:" + b for b in BLOCKS] +
             ["compress_dev", "lin:whole", "lin:blk2", "lin:blk1", "spgemm:whole", "spgemm:blk2", "spgemm:blk1",
              "transpose", "to_complex:whole", "to_complex:blk2"])


# ---- 1. every way to obtain a handle, against the truth ----------------------------------------------------------

def assert_holds(O, H, t):
    inf = H.info()
    assert (inf["nrows_global"], inf["ncols"], inf["row0"], inf["nrows_local"], inf["nnz"]) == \
        (t.nrows_global, t.ncols, t.row0, nloc(t), len(t.ci))
    rp, ci, v = H.export_csr()
    assert np.array_equal(rp, t.rp) and np.array_equal(ci, t.ci)
    assert v.dtype == t.v.dtype and same_bits(v, t.v)
    tup = handle_to_csc_tuple(H)
    assert O.check_matrix(tup[:4] + (np.ascontiguousarray(tup[4].real),)) == 0
    # the same on the row-major arrays themselves (the CSC image of the transpose): columns ascend inside every row
    assert O.check_matrix((inf["ncols"], inf["nrows_local"], rp, ci, np.ascontiguousarray(v.real))) == 0


@pytest.mark.parametrize("name", PRODUCERS)
def test_handle_holds_the_truth(gpu, pkg, O, data, name):
    H, t = produce(gpu, pkg, data["generic"], name)
    assert_holds(O, H, t)


def test_base_matrix_is_what_the_tests_assume(data):
    """the properties the cases above lean on, checked on the oracle's arrays"""
    for d in data.values():
        A = d.get("A")
        lens = np.diff(A.rp)
        assert (A.nrows_global, A.ncols) == (NR, NC) and 55_000 < len(A.ci) < 65_000
        assert all(lens[r] == 0 for r in EMPTY_ROWS) and lens[LONG_ROW] == LONG_LEN == lens.max()
        assert np.diff(d.get("lin").rp).max() <= 512 and np.diff(block(d, "AB", "blk1").rp).max() <= 512
        for name, (r0, r1) in BLOCKS.items():
            assert r0 % 64 or r0 == 0
            assert name in ("zero", "one", "empty") or (r1 - r0) % 256
    assert not np.array_equal(data["generic"].A[4], np.round(data["generic"].A[4]))
    assert np.array_equal(data["integer"].A[4], np.round(data["integer"].A[4]))


def test_from_csc_parts_follow_the_boundary_rule(gpu, pkg, data):
    """block p starts at the first row whose pointer is >= nnz p / nparts; the parts tile the matrix"""
    A = data["generic"].get("A")
    nnz = len(A.ci)
    for nparts in (3, 7):
        at = 0
        for p in range(nparts):
            inf = csc_handle(pkg, data["generic"].A, p, nparts).info()
            target = (nnz * p) // nparts
            first = next(r for r in range(NR + 1) if A.rp[r] >= target) if p else 0  # the rule, spelled out
            assert inf["row0"] == first == at
            at += inf["nrows_local"]
            assert inf["nnz"] == A.rp[at] - A.rp[first]
        assert at == NR


# ---- 2. the exports ----------------------------------------------------------------------------------------------

def windows(t):
    n, lens = nloc(t), np.diff(t.rp)
    w = [(0, 0), (0, 1), (0, n), (n - 1, n)]
    e = np.flatnonzero(lens == 0)
    if len(e):
        w.append((int(e[0]), int(e[0]) + 1))            # one empty row
    long_row = int(np.argmax(lens))
    w.append((max(long_row - 7, 0), min(long_row + 9, n)))  # across the longest row
    return w


@pytest.mark.parametrize("name", ["csr:whole", "csc:1", "csr:blk1", "csr:blk2", "lin:blk2", "spgemm:blk2"])
def test_export_csr_rows_windows(gpu, pkg, data, name):
    H, t = produce(gpu, pkg, data["generic"], name)
    for r0, r1 in windows(t):
        rp, ci, v = H.export_csr_rows(r0, r1)
        w = rows_of(t, r0, r1)
        assert np.array_equal(rp, w.rp) and np.array_equal(ci, w.ci) and same_bits(v, w.v), (r0, r1)


@pytest.mark.parametrize("name", ["csr:whole", "csr:blk2"])
def test_export_csr_rows_capacity_protocol(gpu, pkg, L, data, name):
    H, t = produce(gpu, pkg, data["generic"], name)
    long_row = LONG_ROW - t.row0
    r0, r1 = long_row - 3, long_row + 2
    a, b = int(t.rp[r0]), int(t.rp[r1])
    cnt = b - a
    assert cnt > LONG_LEN and a > 0
    p_i64, p_i32, p_f64 = pkg._ffi.p_i64, pkg._ffi.p_i32, pkg._ffi.p_f64
    # capacity 0: refused, but rowptr already holds the block's offsets (not relative to the window)
    rp = np.full(r1 - r0 + 1, -1, dtype=np.int64)
    assert L.spl_matrix_export_csr_rows(H.handle, r0, r1, p_i64(rp), 0, None, None) == ARG
    assert np.array_equal(rp, t.rp[r0:r1 + 1])
    ci, v = np.full(cnt, -1, dtype=np.int32), np.full(cnt, np.nan)
    rp[:] = -1
    assert L.spl_matrix_export_csr_rows(H.handle, r0, r1, p_i64(rp), cnt - 1, p_i32(ci), p_f64(v)) == ARG
    assert np.array_equal(rp, t.rp[r0:r1 + 1])
    rp[:] = -1
    assert L.spl_matrix_export_csr_rows(H.handle, r0, r1, p_i64(rp), cnt, p_i32(ci), p_f64(v)) == 0
    assert np.array_equal(rp, t.rp[r0:r1 + 1]) and np.array_equal(ci, t.ci[a:b]) and same_bits(v, t.v[a:b])
    # a larger capacity is fine, a window past the block is not, nor one that runs backwards
    assert L.spl_matrix_export_csr_rows(H.handle, r0, r1, p_i64(rp), cnt + 5, p_i32(ci), p_f64(v)) == 0
    big = np.zeros(nloc(t) + 3, dtype=np.int64)
    assert L.spl_matrix_export_csr_rows(H.handle, 0, nloc(t) + 1, p_i64(big), 0, None, None) < 0
    assert L.spl_matrix_export_csr_rows(H.handle, r1, r0, p_i64(big), 0, None, None) < 0
    # a complex handle is refused
    Z = H.to_complex()
    assert L.spl_matrix_export_csr_rows(Z.handle, r0, r1, p_i64(rp), cnt, p_i32(ci), p_f64(v)) < 0


def test_export_csc_whole_is_the_original_tuple(gpu, pkg, data):
    d = data["generic"]
    for H in (csc_handle(pkg, d.A), csr_handle(pkg, d.get("A"))):
        cp, ri, v = H.export_csc()
        assert np.array_equal(cp, d.A[2]) and np.array_equal(ri, d.A[3]) and same_bits(v, d.A[4])


@pytest.mark.parametrize("name", ["csr:blk1", "csr:blk2", "csr:blk3", "csr:one", "csc:1", "csc:2", "lin:blk2", "spgemm:blk1"])
def test_export_csc_of_a_row_block_has_local_rows(gpu, pkg, O, data, name):
    H, t = produce(gpu, pkg, data["generic"], name)
    assert t.row0 > 0
    want = as_csc(O, t)
    cp, ri, v = H.export_csc()
    assert np.array_equal(cp, want[2]) and np.array_equal(ri, want[3]) and same_bits(v, want[4])
    assert len(ri) == 0 or (ri.min() >= 0 and ri.max() < nloc(t))
    inside = np.ones(len(ri), dtype=bool)
    inside[cp[:-1][np.diff(cp) > 0]] = False  # first entry of every non-empty column
    assert np.all(np.diff(ri.astype(np.int64))[inside[1:]] > 0)  # ascending inside each column


@pytest.mark.parametrize("name", ["csr:zero", "csr:empty"])
def test_export_csc_of_a_block_without_entries(gpu, pkg, data, name):
    H, t = produce(gpu, pkg, data["generic"], name)
    cp, ri, v = H.export_csc()
    assert np.array_equal(cp, np.zeros(NC + 1, dtype=np.int64)) and len(ri) == 0 and len(v) == 0


def test_export_csc_refuses_complex(gpu, pkg, L, data):
    Z, t = produce(gpu, pkg, data["generic"], "to_complex:blk2")
    cp, ri, v = np.zeros(NC + 1, dtype=np.int64), np.zeros(len(t.ci), dtype=np.int32), np.zeros(2 * len(t.ci))
    assert L.spl_matrix_export_csc(Z.handle, pkg._ffi.p_i64(cp), pkg._ffi.p_i32(ri), pkg._ffi.p_f64(v)) < 0
    with pytest.raises(Exception):
        Z.export_csc()


# ---- 3. derived handles are consumed, not only read --------------------------------------------------------------

CONSUMED = ["csr:blk2", "csc:1", "lin:blk2", "spgemm:blk1", "transpose", "compress_dev"]
KERNELS = ["stream", "blocked", "sell", "panel", "rounds"]


def select_kernel(H, kernel):
    if kernel == "stream":
        H.set_variant(1)
    elif kernel == "blocked":
        H.build_blocked(300, 12, 0)  # 4 099 columns: the last column block is three columns wide
        H.set_variant(8)
        assert H.spmv_kernel() == 8 and H.info()["blocked_rows"] == 300
    elif kernel == "sell":
        H.set_variant(15)
        assert H.spmv_kernel() == 15 and H.info()["blocked_rows"] == -64
    else:
        H.build_panel(1000, 10, 0, H.PANEL_FORM_ROUNDS if kernel == "rounds" else H.PANEL_FORM_DEFAULT)
        H.set_variant(16)
        assert H.spmv_kernel() == 16 and H.info()["blocked_rows"] == 1000


def products(torch, H, x, y0):
    """mulv, gaxpy, spmv_dev plain and accumulate: ((y = A x) twice, (y0 + A x) twice)"""
    s = torch.cuda.current_stream().cuda_stream
    dx = torch.from_numpy(x).cuda()
    plain = torch.full((len(y0),), np.nan, dtype=torch.float64, device="cuda")  # a plain product overwrites
    acc = torch.from_numpy(y0.copy()).cuda()
    H.spmv_dev(dx.data_ptr(), plain.data_ptr(), stream=s)
    H.spmv_dev(dx.data_ptr(), acc.data_ptr(), accumulate=True, stream=s)
    torch.cuda.synchronize()
    return (H.mulv(x), plain.cpu().numpy()), (H.gaxpy(x, y0.copy()), acc.cpu().numpy())


def reference(O, t, x, y0):
    rp32 = t.rp.astype(np.int32)
    return O.csr_gaxpy32(rp32, t.ci, t.v, x, np.zeros(nloc(t))), O.csr_gaxpy32(rp32, t.ci, t.v, x, y0.copy())


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", CONSUMED)
def test_derived_handle_multiplies(gpu, pkg, O, data, name, kernel):
    torch = gpu
    rng = np.random.default_rng(7)
    H, t = produce(torch, pkg, data["generic"], name)
    select_kernel(H, kernel)
    x, y0 = rng.standard_normal(t.ncols), rng.standard_normal(nloc(t))
    want, want_acc = reference(O, t, x, y0)
    got, got_acc = products(torch, H, x, y0)
    if kernel in ("stream", "blocked", "sell"):  # reference order: the oracle's bits
        for y in got:
            assert same_bits(y, want)
        for y in got_acc:
            assert same_bits(y, want_acc)
        return
    # order-free panels: closeness, the rounding bound of a row's sum in any order, and exact integer data
    rp32, lens = t.rp.astype(np.int32), np.diff(t.rp)
    sabs = O.csr_gaxpy32(rp32, t.ci, np.abs(t.v), np.abs(x), np.zeros(nloc(t)))
    bound = 2.0 * np.maximum(lens, 1) * EPS * sabs
    for y in got:
        print("largest |y - yo| / (2 len eps sum|a x|): %.3g" % float(np.max(np.abs(y - want) / np.maximum(bound, 1e-300))))
        assert O.count_not_close(y, want, 1e-10) == 0
        assert np.all(np.abs(y - want) <= bound)
    for y in got_acc:
        assert O.count_not_close(y, want_acc, 1e-10) == 0
    assert H.panel_errors() == 0
    Hi, ti = produce(torch, pkg, data["integer"], name)
    select_kernel(Hi, kernel)
    xi, yi = rng.integers(-5, 6, ti.ncols).astype(float), rng.integers(-5, 6, nloc(ti)).astype(float)
    want, want_acc = reference(O, ti, xi, yi)
    got, got_acc = products(torch, Hi, xi, yi)
    assert all(same_bits(y, want) for y in got) and all(same_bits(y, want_acc) for y in got_acc)
    assert Hi.panel_errors() == 0


@pytest.mark.parametrize("name", ["csr:zero", "csr:one", "csr:empty"])
def test_degenerate_blocks_multiply(gpu, pkg, O, data, name):
    torch = gpu
    rng = np.random.default_rng(9)
    H, t = produce(torch, pkg, data["generic"], name)
    x, y0 = rng.standard_normal(NC), rng.standard_normal(nloc(t))
    want, want_acc = reference(O, t, x, y0)
    got, got_acc = products(torch, H, x, y0)
    assert all(same_bits(y, want) for y in got) and all(same_bits(y, want_acc) for y in got_acc)


@pytest.mark.parametrize("k", [1, 5, 16, 33])
@pytest.mark.parametrize("name", ["csr:blk2", "lin:blk2", "spgemm:blk1", "transpose"])
def test_derived_handle_spmm(gpu, pkg, O, data, name, k):
    """C = A B and C <- A B + C, row-major dense B: each column bit for bit one axpy of the oracle"""
    torch = gpu
    rng = np.random.default_rng(k)
    H, t = produce(torch, pkg, data["generic"], name)
    m = as_csc(O, t)
    n = nloc(t)
    B, C0 = rng.standard_normal((t.ncols, k)), rng.standard_normal((n, k))
    s = torch.cuda.current_stream().cuda_stream
    dB = torch.from_numpy(B).cuda()
    plain = torch.full((n, k), np.nan, dtype=torch.float64, device="cuda")
    acc = torch.from_numpy(C0.copy()).cuda()
    H.spmm_dev(dB.data_ptr(), plain.data_ptr(), k, stream=s)
    H.spmm_dev(dB.data_ptr(), acc.data_ptr(), k, accumulate=True, stream=s)
    torch.cuda.synchronize()
    want = np.stack([O.axpy(m, B[:, j].copy(), np.zeros(n)) for j in range(k)], axis=1)
    want_acc = np.stack([O.axpy(m, B[:, j].copy(), C0[:, j].copy()) for j in range(k)], axis=1)
    assert same_bits(plain.cpu().numpy(), want)
    assert same_bits(acc.cpu().numpy(), want_acc)


@pytest.mark.parametrize("name", ["to_complex:blk2", "to_complex:whole"])
def test_complex_row_block_multiplies(gpu, pkg, O, data, name):
    rng = np.random.default_rng(11)
    Z, t = produce(gpu, pkg, data["generic"], name)
    assert Z.is_complex
    real = as_csc(O, t._replace(v=np.ascontiguousarray(t.v.real)))
    m = real[:4] + (real[4] + 0j,)
    x = rng.standard_normal(NC) + 1j * rng.standard_normal(NC)
    y0 = rng.standard_normal(nloc(t)) + 1j * rng.standard_normal(nloc(t))
    assert same_bits(Z.mulv(x), O.mulV_z(m, x))
    want = y0.copy()
    O.axpy_z(m, x, want)
    assert same_bits(Z.gaxpy(x, y0.copy()), want)


@pytest.mark.parametrize("blk", [None, "blk2", "blk1"])
def test_lin_of_two_spgemm_results(gpu, pkg, O, data, blk):
    """alpha (A B) + beta (A2 B) without leaving the device, A and A2 whole or the same row block"""
    d = data["generic"]
    HB = csc_handle(pkg, d.B)
    HA, HA2 = (csr_handle(pkg, d.get(w) if blk is None else block(d, w, blk)) for w in ("A", "A2"))
    P1, P2 = HA.spgemm(HB)[0], HA2.spgemm(HB)[0]
    t = d.get("lin_of_products")
    assert_holds(O, P1.lin(ALPHA, P2, BETA), t if blk is None else rows_of(t, *BLOCKS[blk]))


@pytest.mark.parametrize("blk", [None, "blk2", "blk3"])
def test_spgemm_of_a_lin_result_with_a_transpose_result(gpu, pkg, O, data, blk):
    """(alpha A + beta A2) A^T: the left factor a lin result (whole or a row block), the right one a transpose"""
    d = data["generic"]
    HA, HA2 = (csr_handle(pkg, d.get(w) if blk is None else block(d, w, blk)) for w in ("A", "A2"))
    HT = csc_handle(pkg, d.A).transpose()
    HC = HA.lin(ALPHA, HA2, BETA).spgemm(HT)[0]
    t = d.get("product_of_lin")
    assert_holds(O, HC, t if blk is None else rows_of(t, *BLOCKS[blk]))


# ---- 4. refusals the header states -------------------------------------------------------------------------------

def refused(call):
    """call(out) passes `out` as the entry point's output handle: a negative status, and the handle left NULL"""
    h = C.c_void_p(1)
    st = call(C.byref(h))
    return st < 0 and not h.value


def test_refusals(gpu, pkg, L, data):
    d = data["generic"]
    one = (C.c_double * 2)(1.0, 0.0)
    whole_A, blk1, blk2 = (csr_handle(pkg, t) for t in (d.get("A"), block(d, "A", "blk1"), block(d, "A", "blk2")))
    # transpose: whole matrices only
    assert refused(lambda out: L.spl_matrix_transpose(blk2.handle, out))
    # spgemm: B must be whole (the shapes agree: only the row block is wrong)
    B_block = csr_handle(pkg, rows_of(d.get("B"), 100, 3000))
    assert refused(lambda out: L.spl_matrix_spgemm(whole_A.handle, B_block.handle, out, None))
    # lin: same row0 and same nrows_local
    other_row0 = csr_handle(pkg, rows_of(d.get("A2"), 1001, 2003))    # as tall as blk1
    other_height = csr_handle(pkg, rows_of(d.get("A2"), 1000, 2001))  # starts where blk1 starts
    for other in (other_row0, other_height, whole_A):
        assert refused(lambda out: L.spl_matrix_lin(blk1.handle, one, other.handle, one, out))
        assert refused(lambda out: L.spl_matrix_lin(other.handle, one, blk1.handle, one, out))
    # lin: a real and a complex handle
    Z = blk2.to_complex()
    assert refused(lambda out: L.spl_matrix_lin(blk2.handle, one, Z.handle, one, out))
    assert refused(lambda out: L.spl_matrix_lin(Z.handle, one, blk2.handle, one, out))
    # the neighbouring legal calls go through
    blk1.lin(1.0, csr_handle(pkg, block(d, "A2", "blk1")), 1.0)
    Z.lin(1.0, Z, 1.0)
    whole_A.spgemm(csc_handle(pkg, d.B))


# ---- 5. CSR input with unsorted rows -----------------------------------------------------------------------------

def shuffled_rows(t, seed):
    """the same block with the entries of every row permuted (indices and values together)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(nloc(t)), np.diff(t.rp))
    order = np.lexsort((rng.random(len(rows)), rows))
    assert np.array_equal(rows[order], rows) and not np.array_equal(t.ci[order], t.ci)
    return t._replace(ci=t.ci[order], v=t.v[order])


@pytest.mark.parametrize("blk", [None, "blk2"])
def test_from_csr_sorts_unsorted_rows(gpu, pkg, O, data, blk):
    """what the CSC entry points do with unsorted columns (tests/test_gpu_reference_suite.py,
    test_mm_unsorted_input_columns): tolerated, sorted on upload"""
    d = data["generic"]
    t = d.get("A") if blk is None else block(d, "A", blk)
    H = csr_handle(pkg, shuffled_rows(t, 5))
    assert_holds(O, H, t)
    rng = np.random.default_rng(6)
    x, y0 = rng.standard_normal(NC), rng.standard_normal(nloc(t))
    H.set_variant(1)
    want, want_acc = reference(O, t, x, y0)
    got, got_acc = products(gpu, H, x, y0)
    assert all(same_bits(y, want) for y in got) and all(same_bits(y, want_acc) for y in got_acc)
    A2 = d.get("A2") if blk is None else block(d, "A2", blk)
    lin, AB = (d.get(w) if blk is None else block(d, w, blk) for w in ("lin", "AB"))
    assert_holds(O, H.lin(ALPHA, csr_handle(pkg, A2), BETA), lin)
    assert_holds(O, H.lin(ALPHA, csr_handle(pkg, shuffled_rows(A2, 8)), BETA), lin)
    assert_holds(O, H.spgemm(csc_handle(pkg, d.B))[0], AB)
    # as the right factor too: B with unsorted rows
    HB = csr_handle(pkg, shuffled_rows(d.get("B"), 9))
    assert_holds(O, csr_handle(pkg, t).spgemm(HB)[0], AB)
    if blk is None:
        cp, ri, v = H.export_csc()
        assert np.array_equal(cp, d.A[2]) and np.array_equal(ri, d.A[3]) and same_bits(v, d.A[4])


# ---- 6. reserved CUs ---------------------------------------------------------------------------------------------

WIDE_N, WIDE_K, WIDE_ROWS = 6_000_000, 8, 40_000  # a short block of a wide matrix: optimize() chooses an image


@pytest.fixture(scope="module")
def wide(O):
    """x, y0 and the oracle's products of rows [0, 40 000) of random(6 000 000, 8), in 1 000-row windows"""
    x = O.gen_vector(WIDE_N)
    y0 = O.gen_vector(WIDE_ROWS, seed=7)
    want, want_acc, sabs, lens = (np.zeros(WIDE_ROWS) for _ in range(4))
    for r0 in range(0, WIDE_ROWS, 1000):
        rp, ci, v = O.gen_random_csr(WIDE_N, WIDE_K, row0=r0, row1=r0 + 1000)
        w = slice(r0, r0 + 1000)
        want[w] = O.csr_gaxpy32(rp, ci, v, x, np.zeros(1000))
        want_acc[w] = O.csr_gaxpy32(rp, ci, v, x, y0[w].copy())
        sabs[w] = O.csr_gaxpy32(rp, ci, np.abs(v), np.abs(x), np.zeros(1000))
        lens[w] = np.diff(rp)
    return x, y0, want, want_acc, sabs, lens


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("reserved", [0, 1, 37, "above_limit"])
def test_reserved_cus(gpu, pkg, O, wide, reserved, order):
    """the images optimize() lays out for fewer CUs compute the same product; a request above CUs - 8 is clamped
    to CUs - 8 (spmv_cus), not refused"""
    torch = gpu
    x, y0, want, want_acc, sabs, lens = wide
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = cus - 3 if reserved == "above_limit" else reserved
    H = pkg.DeviceMatrix.synthetic("random", WIDE_N, WIDE_K, row0=0, row1=WIDE_ROWS)
    H.set_spmv_order(order)
    H.set_reserved_cus(r)
    H.optimize()
    inf = H.info()
    print("CUs %d, reserved %d, order %d: kernel %d, info %r" % (cus, r, order, H.spmv_kernel(), inf))
    assert (inf["row0"], inf["nrows_local"], inf["ncols"], inf["nnz"]) == (0, WIDE_ROWS, WIDE_N, int(lens.sum()))
    assert H.spmv_kernel() in ((0, 8, 15, 16) if order else (0, 8, 15))  # no order-free image unless asked for
    got, got_acc = products(torch, H, x, y0)
    if order == 0:
        assert all(same_bits(y, want) for y in got) and all(same_bits(y, want_acc) for y in got_acc)
    else:
        bound = 2.0 * np.maximum(lens, 1) * EPS * sabs
        for y in got:
            assert O.count_not_close(y, want, 1e-10) == 0 and np.all(np.abs(y - want) <= bound)
        for y in got_acc:
            assert O.count_not_close(y, want_acc, 1e-10) == 0
        assert H.panel_errors() == 0


def test_reserved_cus_refuses_negative(gpu, pkg, L):
    H = pkg.DeviceMatrix.synthetic("random", 1000, 4)
    assert L.spl_matrix_set_reserved_cus(H.handle, -1) < 0
    with pytest.raises(Exception):
        H.set_reserved_cus(-5)
    H.set_reserved_cus(0)
