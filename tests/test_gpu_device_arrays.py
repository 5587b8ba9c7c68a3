"""Compressed arrays and triples in device memory, in and out of handles: spl_matrix_create_csr_dev, _create_csc_dev,
_compress_dev_wide, _export_csr_dev, _export_csc_dev and DeviceMatrix.from_torch / to_torch.

Every comparison is bitwise.  The expected side is never the new code: it is the handle the host-array route builds from
the same data (DeviceMatrix.from_csr / from_csc / from_csc_complex, read back with export_csr), or the oracle.  The
malformed inputs are small, and the kernels must refuse them by comparison alone: nothing is read through a bad index."""
import ctypes as C

import numpy as np
import pytest

from helpers import handle_to_csc_tuple

pytestmark = pytest.mark.gpu

WIDTHS = {4: np.int32, 8: np.int64}


# ---- data: numpy only ------------------------------------------------------------------------------------------------
def _pattern(rng, nr, nc, k):
    """about k distinct (row, col) pairs in row-major order"""
    if nr == 0 or nc == 0 or k == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    keys = np.unique(rng.integers(0, nr * nc, k))
    return keys // nc, keys % nc


def _values(rng, n, cplx):
    v = rng.normal(size=n)
    return v + 1j * rng.normal(size=n) if cplx else v


def _csr(nr, r, c, v):
    """(rowptr, colidx, val) of entries sorted row-major"""
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nr))]).astype(np.int64)
    return rp, c.astype(np.int64), v


def _csc(nc, r, c, v):
    order = np.lexsort((r, c))
    cp = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=nc))]).astype(np.int64)
    return cp, r[order].astype(np.int64), v[order]


def _cases(rng, cplx):
    """(name, nrows, ncols, rows, cols, values) of the import tests"""
    out = []
    for nr, nc, k in ((1, 1, 1), (37, 129, 400), (5000, 4000, 90_000)):
        r, c = _pattern(rng, nr, nc, k)
        out.append(("%dx%d" % (nr, nc), nr, nc, r, c, _values(rng, len(r), cplx)))
    r, c = _pattern(rng, 37, 129, 400)
    keep = (r >= 3) & (r < 30) & (c != 64)  # empty leading and trailing rows, an empty middle column
    out.append(("holes", 37, 129, r[keep], c[keep], _values(rng, int(keep.sum()), cplx)))
    for nr, nc in ((0, 0), (5, 0), (0, 5)):
        out.append(("%dx%d" % (nr, nc), nr, nc, np.zeros(0, np.int64), np.zeros(0, np.int64), _values(rng, 0, cplx)))
    return out


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return t.data_ptr() if t.numel() else 0


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint64)


def _host_handle(pkg, nr, nc, r, c, v):
    """the parent's route: host arrays, int32 at the seam"""
    cp, ri, cv = _csc(nc, r, c, v)
    M = pkg.Matrix(nc, nr, cp, ri, np.asarray(cv, dtype=np.complex128 if np.iscomplexobj(v) else np.float64))
    return pkg.DeviceMatrix.from_csc_complex(M) if np.iscomplexobj(v) else pkg.DeviceMatrix.from_csc(M)


def _assert_same_handle(Hn, Hh):
    a, b = Hn.info(), Hh.info()
    for key in ("nrows_global", "ncols", "row0", "nrows_local", "nnz"):
        assert a[key] == b[key], key
    assert Hn.is_complex == Hh.is_complex
    (rp, ci, v), (rp0, ci0, v0) = Hn.export_csr(), Hh.export_csr()
    assert rp.dtype == rp0.dtype and np.array_equal(rp, rp0)
    assert np.array_equal(ci, ci0)
    assert np.array_equal(_bits(v), _bits(v0))


def _raw_import(pkg, torch, which, nr, nc, iw, ptr, idx, val, cplx=False):
    """(status, handle value) of spl_matrix_create_{csr,csc}_dev on numpy arrays uploaded as they are"""
    L = pkg._ffi.lib()
    dp, di, dv = _dev(torch, ptr), _dev(torch, idx), _dev(torch, val)
    torch.cuda.synchronize()
    h = C.c_void_p(0x1234)
    fn = L.spl_matrix_create_csr_dev if which == "csr" else L.spl_matrix_create_csc_dev
    st = fn(nr, nc, iw, _ptr(dp), _ptr(di), _ptr(dv), 2 if cplx else 1, C.byref(h))
    return st, h


# ---- import equals the host route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("iw", [4, 8])
def test_import_equals_the_host_route(gpu, pkg, O, iw, cplx):
    torch = gpu
    rng = np.random.default_rng(100 * iw + cplx)
    it = WIDTHS[iw]
    for name, nr, nc, r, c, v in _cases(rng, cplx):
        Hh = _host_handle(pkg, nr, nc, r, c, v)
        rp, ci, rv = _csr(nr, r, c, v)
        drp, dci, drv = _dev(torch, rp.astype(it)), _dev(torch, ci.astype(it)), _dev(torch, rv)
        cp, ri, cv = _csc(nc, r, c, v)
        dcp, dri, dcv = _dev(torch, cp.astype(it)), _dev(torch, ri.astype(it)), _dev(torch, cv)
        torch.cuda.synchronize()
        Hr = pkg.DeviceMatrix.from_csr_dev(nr, nc, _ptr(drp), _ptr(dci), _ptr(drv), index_width=iw, complex=cplx)
        Hc = pkg.DeviceMatrix.from_csc_dev(nr, nc, _ptr(dcp), _ptr(dri), _ptr(dcv), index_width=iw, complex=cplx)
        # the inputs are borrowed for the call only
        for t in (drp, dci, drv, dcp, dri, dcv):
            t.fill_(-1)
        torch.cuda.synchronize()
        _assert_same_handle(Hr, Hh)
        _assert_same_handle(Hc, Hh)
        for H in (Hc, Hr):
            tup = handle_to_csc_tuple(H)
            assert O.check_matrix(tup[:4] + (np.zeros(len(tup[4])),)) == 0, name  # the structure: values are not looked at


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("iw", [4, 8])
def test_no_entries_and_null_arrays(gpu, pkg, iw, cplx):
    torch = gpu
    dp = torch.zeros(5, dtype=torch.int32 if iw == 4 else torch.int64, device="cuda")
    torch.cuda.synchronize()
    Hh = _host_handle(pkg, 4, 4, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, complex if cplx else float))
    for make in (pkg.DeviceMatrix.from_csr_dev, pkg.DeviceMatrix.from_csc_dev):
        _assert_same_handle(make(4, 4, dp.data_ptr(), 0, 0, index_width=iw, complex=cplx), Hh)


# ---- rows that do not ascend ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_unsorted_rows_are_sorted_with_their_values(gpu, pkg, cplx):
    """row lengths on both sides of the sort's regimes (one wavefront up to 64, LDS up to 4096, global above)"""
    torch = gpu
    rng = np.random.default_rng(7 + cplx)
    lens = [1, 2, 64, 65, 4096, 4097]
    nr, nc = len(lens), 6000
    r = np.repeat(np.arange(nr), lens)
    c = np.concatenate([np.sort(rng.choice(nc, n, replace=False)) for n in lens])
    v = np.arange(1, len(r) + 1, dtype=float)  # distinct: a value carried with the wrong key shows
    if cplx:
        v = v - 1j * (v + 0.5)
    Hh = _host_handle(pkg, nr, nc, r, c, v)
    rp = np.concatenate([[0], np.cumsum(lens)])
    perm = np.concatenate([rp[i] + rng.permutation(n) for i, n in enumerate(lens)])
    assert np.any(np.diff(c[perm][rp[4]:rp[5]]) < 0)
    for iw, it in WIDTHS.items():
        drp, dci, dv = _dev(torch, rp.astype(it)), _dev(torch, c[perm].astype(it)), _dev(torch, v[perm])
        torch.cuda.synchronize()
        H = pkg.DeviceMatrix.from_csr_dev(nr, nc, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), index_width=iw, complex=cplx)
        _assert_same_handle(H, Hh)
    # columns whose rows do not ascend: the contract of spl_matrix_create, the transpose orders the row image
    cp, ri, cv = _csc(nc, r, c, v)
    shuffle = np.concatenate([cp[j] + rng.permutation(int(cp[j + 1] - cp[j])) for j in range(nc)]).astype(np.int64)
    dcp, dri, dcv = _dev(torch, cp), _dev(torch, ri[shuffle]), _dev(torch, cv[shuffle])
    torch.cuda.synchronize()
    H = pkg.DeviceMatrix.from_csc_dev(nr, nc, dcp.data_ptr(), dri.data_ptr(), dcv.data_ptr(), index_width=8, complex=cplx)
    _assert_same_handle(H, Hh)


# ---- narrowing is checked, not truncated -----------------------------------------------------------------------------------
def test_out_of_range_indices_and_pointers_are_refused(gpu, pkg):
    torch = gpu
    INVALID = pkg._ffi.SPL_ERROR_invalid_matrix
    rng = np.random.default_rng(3)
    nr, nc = 9, 11
    r, c = _pattern(rng, nr, nc, 40)
    v = _values(rng, len(r), False)
    arrays = {"csr": (_csr(nr, r, c, v), nc), "csc": (_csc(nc, r, c, v), nr)}
    for which, ((ptr, idx, val), nminor) in arrays.items():
        nnz = len(idx)
        assert nnz > 12
        st, h = _raw_import(pkg, torch, which, nr, nc, 8, ptr, idx, val)
        assert st == 0 and h.value  # the arrays are good before they are spoilt
        pkg._ffi.lib().spl_matrix_free(C.byref(h))
        for iw, bad_values in ((8, ((1 << 32) + 3, nminor, -1, 1 << 31, -(1 << 32))), (4, (nminor, -1))):
            for value in bad_values:
                for where in (0, nnz // 2, nnz - 1):
                    spoilt = idx.copy()
                    spoilt[where] = value
                    st, h = _raw_import(pkg, torch, which, nr, nc, iw, ptr.astype(WIDTHS[iw]), spoilt.astype(WIDTHS[iw]), val)
                    assert st == INVALID and not h.value, (which, iw, value, where)
        mid = len(ptr) // 2
        assert ptr[mid] > 0
        back = ptr.copy()
        back[mid] = ptr[mid + 1] + 1  # a step back between mid and mid + 1
        first = ptr.copy()
        first[0] = 1
        negative = ptr.copy()
        negative[1] = -1
        for iw in (4, 8):
            for p in (back, first, negative):
                st, h = _raw_import(pkg, torch, which, nr, nc, iw, p.astype(WIDTHS[iw]), idx.astype(WIDTHS[iw]), val)
                assert st == INVALID and not h.value, (which, iw, p)
        last = ptr.copy()
        last[-1] = 1 << 32  # monotone, and far more entries than the arrays hold: refused before they are read
        st, h = _raw_import(pkg, torch, which, nr, nc, 8, last, idx, val)
        assert st == INVALID and not h.value, which


# ---- COO ---------------------------------------------------------------------------------------------------------------------
def _oracle_compress(O, nr, nc, r, c, v):
    if not np.iscomplexobj(v):
        return O.compress(nr, nc, r, c, v)
    re = O.compress(nr, nc, r, c, v.real.copy())  # complex addition is componentwise
    im = O.compress(nr, nc, r, c, v.imag.copy())
    assert np.array_equal(re[2], im[2]) and np.array_equal(re[3], im[3])
    return (nr, nc, re[2], re[3], re[4] + 1j * im[4])


def _assert_tuple_bits(got, want):
    assert got[0] == want[0] and got[1] == want[1]
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(_bits(got[4]), _bits(np.asarray(want[4], dtype=got[4].dtype)))


def _triples(rng, kind, cplx):
    if kind == "duplicates":
        nr = nc = 30
        r, c = rng.integers(0, nr, 4000), rng.integers(0, nc, 4000)
        v = _values(rng, 4000, cplx)  # not exactly summable: the order of the sums shows
        v[::7] = 0.0
    else:
        nr, nc = 200, 150
        r, c = _pattern(rng, nr, nc, 300)
        p = rng.permutation(len(r))
        r, c = r[p], c[p]
        v = _values(rng, len(r), cplx)
        v[::5] = 0.0  # explicit zeros are kept
    return nr, nc, r, c, v


@pytest.mark.parametrize("kind", ["duplicates", "distinct"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("iw", [4, 8])
def test_compress_wide_against_the_oracle(gpu, pkg, O, iw, cplx, kind):
    torch = gpu
    rng = np.random.default_rng(iw + 2 * cplx)
    nr, nc, r, c, v = _triples(rng, kind, cplx)
    want = _oracle_compress(O, nr, nc, r, c, v)
    if kind == "distinct":
        assert len(want[3]) == len(r) and np.any(want[4] == 0)
    dr, dc, dv = _dev(torch, r.astype(WIDTHS[iw])), _dev(torch, c.astype(WIDTHS[iw])), _dev(torch, v)
    torch.cuda.synchronize()
    L = pkg._ffi.lib()
    h = C.c_void_p()
    bad = C.c_int64(-1)
    st = L.spl_matrix_compress_dev_wide(nr, nc, len(r), iw, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), 2 if cplx else 1,
                                        C.byref(h), C.byref(bad))
    assert st == 0 and h.value
    H = pkg.DeviceMatrix(h.value)
    _assert_tuple_bits(handle_to_csc_tuple(H), want)
    if iw == 4 and not cplx:  # the bits of spl_matrix_compress_dev on the same arrays
        _assert_same_handle(H, pkg.DeviceMatrix.compress_dev(nr, nc, len(r), dr.data_ptr(), dc.data_ptr(), dv.data_ptr()))
    # the method reaches the same symbol
    _assert_same_handle(pkg.DeviceMatrix.compress_dev(nr, nc, len(r), dr.data_ptr(), dc.data_ptr(), dv.data_ptr(),
                                                      index_width=iw, complex=cplx), H)


@pytest.mark.parametrize("iw", [4, 8])
def test_compress_wide_reports_rows_before_columns(gpu, pkg, iw):
    torch = gpu
    rng = np.random.default_rng(5)
    nr, nc, n = 20, 30, 64
    r, c = rng.integers(0, nr, n), rng.integers(0, nc, n)
    v = _values(rng, n, False)
    L = pkg._ffi.lib()
    for bad_row, bad_col in ((nr, nc), (-1, -1)) + ((((1 << 32) + 2, (1 << 32) + 2),) if iw == 8 else ()):
        rr, cc = r.copy(), c.copy()
        rr[17] = bad_row
        cc[5] = bad_col
        dr, dc, dv = _dev(torch, rr.astype(WIDTHS[iw])), _dev(torch, cc.astype(WIDTHS[iw])), _dev(torch, v)
        torch.cuda.synchronize()
        h = C.c_void_p(0x1234)
        bad = C.c_int64(-1)
        st = L.spl_matrix_compress_dev_wide(nr, nc, n, iw, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), 1, C.byref(h), C.byref(bad))
        assert st == pkg._ffi.SPL_ERROR_index_out_of_bounds and not h.value and bad.value == 17
        good = _dev(torch, r.astype(WIDTHS[iw]))
        torch.cuda.synchronize()
        st = L.spl_matrix_compress_dev_wide(nr, nc, n, iw, good.data_ptr(), dc.data_ptr(), dv.data_ptr(), 1, C.byref(h), C.byref(bad))
        assert st == pkg._ffi.SPL_ERROR_index_out_of_bounds and not h.value and bad.value == 5  # rows good: the column


# ---- export --------------------------------------------------------------------------------------------------------------------
CANARY = 8


def _export(torch, H, which, iw):
    """the three arrays of H.export_{csr,csc}_dev read back, after the canaries behind them were checked"""
    inf = H.info()
    vw = 2 if H.is_complex else 1
    np_ = (inf["nrows_local"] if which == "csr" else inf["ncols"]) + 1
    it = torch.int32 if iw == 4 else torch.int64
    ptr = torch.full((np_ + CANARY,), -77, dtype=it, device="cuda")
    idx = torch.full((inf["nnz"] + CANARY,), -77, dtype=it, device="cuda")
    val = torch.full((inf["nnz"] * vw + CANARY,), -77.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    (H.export_csr_dev if which == "csr" else H.export_csc_dev)(ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), index_width=iw)
    ptr, idx, val = ptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()
    assert np.all(ptr[np_:] == -77) and np.all(idx[inf["nnz"]:] == -77) and np.all(val[inf["nnz"] * vw:] == -77.0)
    return ptr[:np_], idx[:inf["nnz"]], val[:inf["nnz"] * vw]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("iw", [4, 8])
def test_export_equals_the_host_exports(gpu, pkg, iw, cplx):
    torch = gpu
    rng = np.random.default_rng(11)
    for nr, nc, k in ((37, 129, 400), (5000, 4000, 90_000), (3, 4, 0)):
        r, c = _pattern(rng, nr, nc, k)
        H = _host_handle(pkg, nr, nc, r, c, _values(rng, len(r), cplx))
        rp, ci, v = H.export_csr()
        p, i, x = _export(torch, H, "csr", iw)
        assert np.array_equal(p, rp) and np.array_equal(i, ci) and np.array_equal(_bits(x), _bits(v))
        _, _, cp, ri, cv = handle_to_csc_tuple(H)
        p, i, x = _export(torch, H, "csc", iw)
        assert np.array_equal(p, cp) and np.array_equal(i, ri) and np.array_equal(_bits(x), _bits(cv))
        if not cplx:
            cp0, ri0, cv0 = H.export_csc()
            assert np.array_equal(p, cp0) and np.array_equal(i, ri0) and np.array_equal(_bits(x), _bits(cv0))


@pytest.mark.parametrize("iw", [4, 8])
def test_export_csr_dev_serves_row_blocks(gpu, pkg, iw):
    torch = gpu
    rng = np.random.default_rng(13)
    nr, nc = 37, 129
    r, c = _pattern(rng, nr, nc, 400)
    cp, ri, cv = _csc(nc, r, c, _values(rng, len(r), False))
    H = pkg.DeviceMatrix.from_csc(pkg.Matrix(nc, nr, cp, ri, cv), part=1, nparts=3)
    inf = H.info()
    assert 0 < inf["row0"] and inf["nrows_local"] < nr and inf["nnz"] > 0
    rp, ci, v = H.export_csr()
    p, i, x = _export(torch, H, "csr", iw)
    assert p[0] == 0 and np.array_equal(p, rp) and np.array_equal(i, ci) and np.array_equal(_bits(x), _bits(v))
    with pytest.raises(ValueError):
        H.to_torch()


# ---- bits ----------------------------------------------------------------------------------------------------------------------
def test_values_are_moved_as_bits(gpu, pkg):
    torch = gpu
    special = np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001,
                        0x7FF4000000000ABC, 0xFFFFFFFFFFFFFFFF, 0x0000000000000001, 0x3FF0000000000000], dtype=np.uint64)
    nr, nc = 4, 5
    r = np.array([0, 0, 1, 1, 2, 2, 3, 3])
    c = np.array([0, 3, 1, 4, 0, 2, 2, 4])
    v = special.view(np.float64)
    rp, ci, _ = _csr(nr, r, c, v)
    cp, ri, cv = _csc(nc, r, c, v)
    drp, dci, dv = _dev(torch, rp), _dev(torch, ci), torch.from_numpy(special.view(np.int64)).cuda()
    dcp, dri, dcv = _dev(torch, cp), _dev(torch, ri), torch.from_numpy(_bits(cv).view(np.int64)).cuda()
    torch.cuda.synchronize()
    Hr = pkg.DeviceMatrix.from_csr_dev(nr, nc, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), index_width=8)
    Hc = pkg.DeviceMatrix.from_csc_dev(nr, nc, dcp.data_ptr(), dri.data_ptr(), dcv.data_ptr(), index_width=8)
    for H in (Hr, Hc):
        assert np.array_equal(_bits(_export(torch, H, "csr", 8)[2]), special)
        assert np.array_equal(_bits(_export(torch, H, "csc", 4)[2]), _bits(cv))
    # packed pairs: the same eight words as four complex entries
    rz, cz = np.array([0, 1, 2, 3]), np.array([1, 0, 3, 2])
    rpz, ciz, _ = _csr(nr, rz, cz, np.zeros(4))
    drpz, dciz = _dev(torch, rpz), _dev(torch, ciz)
    torch.cuda.synchronize()
    Hz = pkg.DeviceMatrix.from_csr_dev(nr, nc, drpz.data_ptr(), dciz.data_ptr(), dv.data_ptr(), index_width=8, complex=True)
    assert Hz.is_complex
    assert np.array_equal(_bits(_export(torch, Hz, "csr", 4)[2]), special)
    order = np.argsort(cz, kind="stable")
    assert np.array_equal(_bits(_export(torch, Hz, "csc", 8)[2]).reshape(4, 2), special.reshape(4, 2)[order])
    # the compress of distinct triples moves them too
    dr, dc = _dev(torch, r), _dev(torch, c)
    torch.cuda.synchronize()
    H = pkg.DeviceMatrix.compress_dev(nr, nc, 8, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), index_width=8)
    assert np.array_equal(_bits(_export(torch, H, "csr", 8)[2]), special)


# ---- the handles are ordinary ----------------------------------------------------------------------------------------------------
def _imported(torch, pkg, nr, nc, r, c, v, iw=8):
    rp, ci, rv = _csr(nr, r, c, v)
    drp, dci, dv = _dev(torch, rp.astype(WIDTHS[iw])), _dev(torch, ci.astype(WIDTHS[iw])), _dev(torch, rv)
    torch.cuda.synchronize()
    return pkg.DeviceMatrix.from_csr_dev(nr, nc, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), index_width=iw,
                                         complex=np.iscomplexobj(v))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_an_imported_handle_is_an_ordinary_handle(gpu, pkg, O, cplx):
    torch = gpu
    rng = np.random.default_rng(17 + cplx)
    nr, nc, nb = 300, 257, 190
    ra, ca = _pattern(rng, nr, nc, 4000)
    rb, cb = _pattern(rng, nr, nc, 2500)
    r2, c2 = _pattern(rng, nc, nb, 3000)
    va, vb, v2 = _values(rng, len(ra), cplx), _values(rng, len(rb), cplx), _values(rng, len(r2), cplx)
    Hi, Hh = _imported(torch, pkg, nr, nc, ra, ca, va), _host_handle(pkg, nr, nc, ra, ca, va)
    HB, H2 = _host_handle(pkg, nr, nc, rb, cb, vb), _host_handle(pkg, nc, nb, r2, c2, v2)
    tup = lambda n, m, r, c, v: (n, m) + _csc(m, r, c, v)  # noqa: E731
    A, B, B2 = tup(nr, nc, ra, ca, va), tup(nr, nc, rb, cb, vb), tup(nc, nb, r2, c2, v2)
    # spmv_many_dev, k = 3
    dt = torch.complex128 if cplx else torch.float64
    X = _dev(torch, _values(rng, 3 * nc, cplx).reshape(3, nc))
    Y = [torch.zeros((3, nr), dtype=dt, device="cuda") for _ in range(2)]
    for H, y in zip((Hi, Hh), Y):
        H.spmv_many_dev(X.data_ptr(), nc, y.data_ptr(), nr, 3, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y[0].cpu().numpy().ravel()), _bits(Y[1].cpu().numpy().ravel()))
    assert np.any(Y[1].cpu().numpy() != 0)
    # lin and spgemm between an imported and a host-built handle
    if cplx:
        al, be = 1.25 + 0.75j, -0.5 + 2.0j
        _assert_tuple_bits(handle_to_csc_tuple(Hi.lin(al, HB, be)), O.lin_z(al, A, be, B))
        _assert_tuple_bits(handle_to_csc_tuple(HB.lin(al, Hi, be)), O.lin_z(al, B, be, A))
        _assert_tuple_bits(handle_to_csc_tuple(Hi.spgemm(H2)[0]), O.mm_z(A, B2))
    else:
        _assert_tuple_bits(handle_to_csc_tuple(Hi.lin(2.0, HB, -1.5)), O.lin(2.0, A, -1.5, B))
        _assert_tuple_bits(handle_to_csc_tuple(HB.lin(2.0, Hi, -1.5)), O.lin(2.0, B, -1.5, A))
        _assert_tuple_bits(handle_to_csc_tuple(Hi.spgemm(H2)[0]), O.mm(A, B2))


def _laplacian(m):
    """5-point Laplacian of side m as sorted CSR arrays"""
    n = m * m
    i, j = np.divmod(np.arange(n), m)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [np.full(n, 4.0)]
    for ok, off in ((i > 0, -m), (i < m - 1, m), (j > 0, -1), (j < m - 1, 1)):
        rows.append(np.arange(n)[ok])
        cols.append(np.arange(n)[ok] + off)
        vals.append(np.full(int(ok.sum()), -1.0))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((c, r))
    return n, r[order], c[order], v[order]


def test_lu_of_a_matrix_imported_from_a_torch_tensor(gpu, pkg):
    """symbolic_dev / numeric_dev / solve_many_dev with NULL host arrays: the bits of the host-built handle's"""
    torch = gpu
    U = pkg.umfpack
    n, r, c, v = _laplacian(12)
    rp, ci, rv = _csr(n, r, c, v)
    t = torch.sparse_csr_tensor(_dev(torch, rp), _dev(torch, ci), _dev(torch, rv), size=(n, n))
    Hs = (pkg.DeviceMatrix.from_torch(t), _host_handle(pkg, n, n, r, c, v))
    _assert_same_handle(*Hs)
    rng = np.random.default_rng(19)
    B = _dev(torch, rng.normal(size=(3, n)))
    X = []
    for H in Hs:
        f = U.factorDevice(H, U.analyzeDevice(H))
        X.append(U.linearSolveManyDevice_(f, U.UmfpackNormal, None, B).cpu().numpy())
    assert np.array_equal(_bits(X[0].ravel()), _bits(X[1].ravel()))
    dense = np.zeros((n, n))
    dense[r, c] = v
    assert np.max(np.abs(dense @ X[0].T - B.cpu().numpy().T)) < 1e-10  # and they are solutions


# ---- torch ---------------------------------------------------------------------------------------------------------------------
def _torch_parts(torch, t):
    if t.layout == torch.sparse_csr:
        return t.crow_indices(), t.col_indices(), t.values()
    return t.ccol_indices(), t.row_indices(), t.values()


def _values_bits(torch, x):
    x = x.clone()  # values() of a compressed tensor is an alias that view_as_real refuses
    return (torch.view_as_real(x) if x.is_complex() else x).contiguous().view(torch.int64)


@pytest.mark.parametrize("cplx", [False, True], ids=["float64", "complex128"])
@pytest.mark.parametrize("iw", [4, 8], ids=["int32", "int64"])
@pytest.mark.parametrize("layout", ["csr", "csc"])
def test_torch_round_trip(gpu, pkg, layout, iw, cplx):
    torch = gpu
    rng = np.random.default_rng(23)
    nr, nc = 211, 300
    r, c = _pattern(rng, nr, nc, 5000)
    v = _values(rng, len(r), cplx)
    it = torch.int32 if iw == 4 else torch.int64
    layouts = {"csr": torch.sparse_csr, "csc": torch.sparse_csc}
    arrays = {"csr": _csr(nr, r, c, v), "csc": _csc(nc, r, c, v)}
    make = {"csr": torch.sparse_csr_tensor, "csc": torch.sparse_csc_tensor}
    p, i, x = arrays[layout]
    t = make[layout](_dev(torch, p).to(it), _dev(torch, i).to(it), _dev(torch, x), size=(nr, nc))
    H = pkg.DeviceMatrix.from_torch(t)
    _assert_same_handle(H, _host_handle(pkg, nr, nc, r, c, v))
    for out in ("csr", "csc"):
        back = H.to_torch(layouts[out], it)
        assert back.layout == layouts[out] and tuple(back.shape) == (nr, nc) and back.device == t.device
        assert back.dtype == (torch.complex128 if cplx else torch.float64)
        want = t if out == layout else make[out](*[_dev(torch, a) for a in arrays[out]], size=(nr, nc))
        for got, exp in zip(_torch_parts(torch, back)[:2], _torch_parts(torch, want)[:2]):
            assert got.dtype == it and torch.equal(got, exp.to(it))
        assert torch.equal(_values_bits(torch, back.values()), _values_bits(torch, want.values()))
    default = H.to_torch()
    assert default.layout == torch.sparse_csr and default.crow_indices().dtype == torch.int64


@pytest.mark.parametrize("cplx", [False, True], ids=["float64", "complex128"])
@pytest.mark.parametrize("iw", [4, 8], ids=["int32", "int64"])
def test_from_torch_coo_sums_duplicates_like_compress(gpu, pkg, O, iw, cplx):
    torch = gpu
    rng = np.random.default_rng(29)
    nr, nc, r, c, v = _triples(rng, "duplicates", cplx)
    idx = _dev(torch, np.stack([r, c])).to(torch.int32 if iw == 4 else torch.int64)
    t = torch.sparse_coo_tensor(idx, _dev(torch, v), size=(nr, nc))
    assert not t.is_coalesced()
    H = pkg.DeviceMatrix.from_torch(t)
    _assert_tuple_bits(handle_to_csc_tuple(H), _oracle_compress(O, nr, nc, r, c, v))
    # an index tensor that is not contiguous is made so on the device
    strided = torch.sparse_coo_tensor(_dev(torch, np.stack([r, r, c, c]))[::2].to(idx.dtype), _dev(torch, v), size=(nr, nc))
    _assert_same_handle(pkg.DeviceMatrix.from_torch(strided), H)


def test_from_torch_refuses_on_the_gpu_too(gpu, pkg):
    torch = gpu
    crow, col = torch.tensor([0, 1, 2], device="cuda"), torch.tensor([0, 1], device="cuda")
    with pytest.raises(TypeError):
        pkg.DeviceMatrix.from_torch(torch.sparse_csr_tensor(crow, col, torch.ones(2, device="cuda"), size=(2, 2)))
    with pytest.raises(TypeError):
        pkg.DeviceMatrix.from_torch(torch.eye(2, dtype=torch.float64, device="cuda"))
    hybrid = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]], device="cuda"),
                                     torch.ones(2, 3, dtype=torch.float64, device="cuda"), size=(2, 2, 3))
    with pytest.raises(ValueError):
        pkg.DeviceMatrix.from_torch(hybrid)
