"""shared generators for the property tests — the reference's QuickCheck
generators (sparse-linear/tests/Test/LinearAlgebra.hs:17-38) as hypothesis strategies"""
import numpy as np
from hypothesis import strategies as st

# arbdim = arbitrary `suchThat` (> 0) (Test/LinearAlgebra.hs:26-27); QuickCheck sizes
# stay small, so do these
arbdim = st.integers(min_value=1, max_value=12)
# element type of almost every reference property is Int: integer-valued doubles
# keep every sum and product exact, so `===` stays meaningful in fp64
arbval = st.integers(min_value=-50, max_value=50).map(float)


@st.composite
def arbitrary_triples(draw, nr, nc):
    """nr*nc/4 + 1 uniformly random (r, c, x) triples (Test/LinearAlgebra.hs:29-38)"""
    k = nr * nc // 4 + 1
    rows = draw(st.lists(st.integers(0, nr - 1), min_size=k, max_size=k))
    cols = draw(st.lists(st.integers(0, nc - 1), min_size=k, max_size=k))
    vals = draw(st.lists(arbval, min_size=k, max_size=k))
    return list(zip(rows, cols, vals))


@st.composite
def arbitrary_dims_triples(draw):
    nr, nc = draw(arbdim), draw(arbdim)
    return nr, nc, draw(arbitrary_triples(nr, nc))


def csc_tuple_to_scipy(m):
    import scipy.sparse as sp
    nrows, ncols, p, i, x = m
    return sp.csc_matrix((np.asarray(x), np.asarray(i), np.asarray(p)), shape=(nrows, ncols))


def mat_to_tuple(M):
    """product Matrix -> oracle tuple"""
    return (M.nrows, M.ncols, M.pointers, M.indices, M.values)


def tuple_to_mat(pkg, m):
    nrows, ncols, p, i, x = m
    return pkg.Matrix(ncols, nrows, p, i, x)


def tuples_equal(a, b):
    return (a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
            and np.array_equal(a[4], b[4]))


def handle_to_csc_tuple(H):
    """(nrows_local, ncols, colptr, rowidx, values) of a device handle's block, local row ids: its CSR arrays are the
    CSC arrays of the transpose, so transpose back on the host side with a stable sort (order inside columns
    preserved)"""
    inf = H.info()
    rp, ci, v = H.export_csr()
    nr, nc = inf["nrows_local"], inf["ncols"]
    rows = np.repeat(np.arange(nr, dtype=np.int64), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    cp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=nc))]).astype(np.int64)
    return (nr, nc, cp, rows[order], v[order])


# ---- the componentwise backward error of a delivered solution, evaluated exactly (tests/first_walk_cases.py) -------
def two_product(a, b):
    """p, e with p = fl(a * b) and a * b == p + e exactly, elementwise (Veltkamp's split, Dekker's product: no fused
    multiply-add needed; exact unless a partial product over- or underflows, which the unit-sized test data cannot do)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b  # 2^27 + 1
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def real_embedding(S):
    """the 2n x 2n real matrix of a complex S for interleaved unknowns (re x_0, im x_0, re x_1, ...): block (i, j) is
    [[Re, -Im], [Im, Re]] (csrc/umfpack_zi.hip); zeros of either part are not stored"""
    import scipy.sparse as sp
    C = sp.coo_matrix(S)
    n = C.shape[0]
    r, c, re, im = C.row, C.col, C.data.real, C.data.imag
    E = sp.csr_matrix((np.concatenate([re, -im, im, re]),
                       (np.concatenate([2 * r, 2 * r, 2 * r + 1, 2 * r + 1]),
                        np.concatenate([2 * c, 2 * c + 1, 2 * c, 2 * c + 1]))), shape=(2 * n, 2 * C.shape[1]))
    E.eliminate_zeros()
    return E


def exact_backward_error(S, x, b):
    """max_i |r_i| / (sum_k |a_ik| |x_k| + |b_i|) with r = b - S x, for a scipy matrix S: every product is split into
    its rounded value and its rounding error, and each row is summed by math.fsum, so r_i and the denominator are the
    correctly rounded values of the exact ones — no extended type of the host, no rounding of a plain S @ x - b.
    Complex data is measured on the real embedding (real_embedding above).  A row with r_i != 0 over a zero
    denominator gives inf.  x, b: one vector each (the result is a float), or k of them as a list or the rows of a
    2-D array (a list of k floats)."""
    import math

    import scipy.sparse as sp
    if not isinstance(x, np.ndarray) or x.ndim == 2:
        return [exact_backward_error(S, np.asarray(xc), np.asarray(bc)) for xc, bc in zip(x, b)]
    if np.iscomplexobj(S.data if sp.issparse(S) else S) or np.iscomplexobj(x) or np.iscomplexobj(b):
        S = real_embedding(sp.csr_matrix(S).astype(np.complex128))
        x = np.ascontiguousarray(x, dtype=np.complex128).view(np.float64)
        b = np.ascontiguousarray(b, dtype=np.complex128).view(np.float64)
    S = sp.csr_matrix(S)
    x, b = np.asarray(x, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert S.shape == (len(b), len(x))
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(b))):
        return float("inf")
    p, e = two_product(S.data, x[S.indices])
    ap, ae = np.abs(p), np.where(p < 0.0, -e, e)  # |a x| == |p| + sign(p) e exactly (|e| <= ulp(p) / 2)
    ptr = S.indptr.tolist()
    p, e, ap, ae, bl = p.tolist(), e.tolist(), ap.tolist(), ae.tolist(), b.tolist()
    worst = 0.0
    for i in range(S.shape[0]):
        lo, hi = ptr[i], ptr[i + 1]
        r = abs(math.fsum([bl[i]] + [-v for v in p[lo:hi]] + [-v for v in e[lo:hi]]))
        if r == 0.0:
            continue
        den = math.fsum([abs(bl[i])] + ap[lo:hi] + ae[lo:hi])
        w = r / den if den > 0.0 else float("inf")
        if not w <= worst:
            worst = w
    return worst


# ---- the order-free panel SpMV (csrc/spmv_panel.hip): what every form has to meet -------------------------
EPS = np.finfo(float).eps


def panel_stream(torch):
    return torch.cuda.current_stream().cuda_stream


def panel_run(torch, H, x):
    n = H.info()["nrows_local"]
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    H.spmv_dev(x.data_ptr(), y.data_ptr(), stream=panel_stream(torch))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def panel_check(torch, O, H, ncols):
    """the three-part contract on whatever H holds: product, rounding bound, accumulate form"""
    nrows = H.info()["nrows_local"]
    rp, ci, v = H.export_csr()
    rp32 = rp.astype(np.int32)
    xh = O.gen_vector(ncols)
    x = torch.from_numpy(xh).cuda()
    y = panel_run(torch, H, x)
    yo = np.zeros(nrows)
    O.csr_gaxpy32(rp32, ci, v, xh, yo)
    bad = O.count_not_close(y, yo, 1e-10)
    sabs = np.zeros(nrows)
    O.csr_gaxpy32(rp32, ci, np.abs(v), np.abs(xh), sabs)  # sum |a x| per row
    lens = np.diff(rp)
    excess = np.abs(y - yo) - 2.0 * np.maximum(lens, 1) * EPS * sabs
    print("not close at 1e-10: %d; largest |y - yo| / (2 len eps sum|a x|): %.3g"
          % (bad, float(np.max(np.abs(y - yo) / np.maximum(2.0 * np.maximum(lens, 1) * EPS * sabs, 1e-300)))))
    assert bad == 0
    assert np.all(excess <= 0.0)
    y0 = O.gen_vector(nrows, seed=7)
    yd = torch.from_numpy(y0.copy()).cuda()
    H.spmv_dev(x.data_ptr(), yd.data_ptr(), accumulate=True, stream=panel_stream(torch))
    torch.cuda.synchronize()
    ya = y0.copy()
    O.csr_gaxpy32(rp32, ci, v, xh, ya)
    assert O.count_not_close(yd.cpu().numpy(), ya, 1e-10) == 0
    assert H.panel_errors() == 0
