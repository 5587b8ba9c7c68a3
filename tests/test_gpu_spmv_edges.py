"""Every SpMV kernel family on signed data with cancellation, on 400 binades of dynamic range, on overflowing and
subnormal products and on infinities, NaNs and stored zeros (tests/spmv_edge_cases.py: two small matrices, an exact
reference, rules that come from the arithmetic).  Every image format pads — SELL with (column 0, value 0) behind a
length mask, the panel image with (block column 0, dummy row, value 0), the blocked image with slack entries — and
0 * x[pad column] must never reach a real row: one infinite x[j] turns every row NaN that a broken mask lets it reach.

Every case asserts which kernel runs before it looks at a value, runs y = A x into a NaN-prefilled y and y <- A x + y0,
and under `poison` runs the same kernel again with the poison replaced by finite values: rows that store no poisoned
column must not change.  Reference-order kernels must give the oracle's bits wherever it is not NaN; the order-free
panel forms the bound gamma_n sum |a x| per row and the oracle's class (finite, +inf, -inf, NaN) everywhere."""
import numpy as np
import pytest

import spmv_edge_cases as E
from helpers import panel_stream, tuple_to_mat

pytestmark = pytest.mark.gpu

VALUES = ("signed", "wide", "huge", "poison")

_handles = {}
_refs = {}


def _handle(pkg, matrix, values):
    """one handle per matrix and set of matrix values for the whole module (poison shares signed's values): set_variant
    and build_* replace the kernel and the image, the CSR arrays stay"""
    c = E.case(matrix, values)
    base = c.clean or c
    key = (matrix, base.name)
    if key not in _handles:
        M = tuple_to_mat(pkg, base.csc())
        _handles[key] = pkg.DeviceMatrix.from_csc_complex(M) if base.is_complex else pkg.DeviceMatrix.from_csc(M)
    return _handles[key]


def _oracle(O, c, accumulate):
    """the oracle's result, computed once per case"""
    key = (c.P.name, c.name, accumulate)
    if key not in _refs:
        A = c.csc()
        if c.is_complex:
            y = c.y0.copy() if accumulate else np.zeros(c.P.nrows, dtype=np.complex128)
            O.axpy_z(A, c.x, y)
        else:
            y = O.axpy(A, c.x, c.y0) if accumulate else O.mulV(A, c.x)
        y.setflags(write=False)
        _refs[key] = y
    return _refs[key]


def _prefilled(torch, c, accumulate, shape=None):
    """y0 for the accumulate form, NaN everywhere for y = A x"""
    if accumulate:
        return torch.from_numpy(np.array(c.y0)).cuda()
    dt = torch.complex128 if c.is_complex else torch.float64
    return torch.full(shape or (c.P.nrows,), float("nan"), dtype=dt, device="cuda")


def _spmv(torch, H, c, accumulate):
    x = torch.from_numpy(np.array(c.x)).cuda()
    y = _prefilled(torch, c, accumulate)
    H.spmv_dev(x.data_ptr(), y.data_ptr(), accumulate=accumulate, stream=panel_stream(torch))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _verify(O, run, c, mode, tree_over=None, forms=(False, True)):
    for accumulate in forms:
        got = run(c, accumulate)
        clean = run(c.clean, accumulate) if c.clean is not None else None
        ref = _oracle(O, c, accumulate) if mode == "reference" else None
        E.check(got, c, accumulate, mode, ref=ref, clean_got=clean, tree_over=tree_over)


def _verify_handle(torch, O, H, c, mode, tree_over=None):
    _verify(O, lambda case, accumulate: _spmv(torch, H, case, accumulate), c, mode, tree_over)


def _same_bits(a, b):
    """bit for bit where neither is NaN, NaN in the same places"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


# ---- reference order, the edge matrix ------------------------------------------------------------------------------
STREAM = (1, 2, 3, 4, 5, 6, 9, 10, 11)


@pytest.mark.parametrize("variant,values", [(v, s) for v in STREAM for s in VALUES] + [(1, "tiny")])
def test_stream_variants(gpu, pkg, O, variant, values):
    """the CSR-stream kernel in every instantiation: the reference's bits, but for the documented wavefront tree on the
    row of 700 entries, which keeps the bound and the class"""
    H = _handle(pkg, "edge", values)
    H.set_variant(variant)
    assert H.spmv_kernel() == variant
    _verify_handle(gpu, O, H, E.case("edge", values), "reference", tree_over=E.STREAM_CHUNK)


@pytest.mark.parametrize("values", VALUES)
def test_subwavefront_variant(gpu, pkg, O, values):
    """variant 7 sums a row in a 16-lane tree (csrc/spmv.hip): the order-free rules"""
    H = _handle(pkg, "edge", values)
    H.set_variant(7)
    assert H.spmv_kernel() == 7
    _verify_handle(gpu, O, H, E.case("edge", values), "free")


BLOCKED = [(64, 8, 0), (500, 12, 4), (64, 8, -1)]


@pytest.mark.parametrize("rows_per_panel,cols_log2,unroll,values",
                         [b + (s,) for b in BLOCKED for s in VALUES] + [BLOCKED[0] + ("tiny",)])
def test_blocked_image(gpu, pkg, O, rows_per_panel, cols_log2, unroll, values):
    H = _handle(pkg, "edge", values)
    H.build_blocked(rows_per_panel, cols_log2, unroll)
    H.set_variant(8)
    assert H.spmv_kernel() == 8 and H.info()["blocked_rows"] == rows_per_panel
    _verify_handle(gpu, O, H, E.case("edge", values), "reference")


@pytest.mark.parametrize("values", VALUES)
def test_default_after_optimize(gpu, pkg, O, values):
    """a handle of its own: what optimize() chooses must not depend on the images other cases built"""
    c = E.case("edge", values)
    H = pkg.DeviceMatrix.from_csc(tuple_to_mat(pkg, c.csc()))
    H.optimize()
    assert H.spmv_kernel() == 0       # a small matrix keeps the CSR-stream kernel, reference order
    _verify_handle(gpu, O, H, c, "reference", tree_over=E.STREAM_CHUNK)
    H.free()


@pytest.mark.parametrize("values", VALUES)
def test_spmm_three_columns(gpu, pkg, O, values):
    """spmm_dev with k = 3, the case's x (the poisoned one) in column 1 only: column 1 is the case, and columns 0 and 2
    equal the unpoisoned run bit for bit"""
    torch = gpu
    c = E.case("edge", values)
    other = c.clean or c
    H = _handle(pkg, "edge", values)

    def run(middle, accumulate):
        B = torch.from_numpy(np.stack([other.x, middle.x, other.x], axis=1)).cuda()
        if accumulate:
            C = torch.from_numpy(np.stack([other.y0, middle.y0, other.y0], axis=1)).cuda()
        else:
            C = _prefilled(torch, c, False, shape=(c.P.nrows, 3))
        H.spmm_dev(B.data_ptr(), C.data_ptr(), 3, accumulate=accumulate, stream=panel_stream(torch))
        torch.cuda.synchronize()
        return C.cpu().numpy()

    for accumulate in (False, True):
        got, plain = run(c, accumulate), run(other, accumulate)
        E.check(got[:, 1].copy(), c, accumulate, "reference", ref=_oracle(O, c, accumulate),
                clean_got=plain[:, 1].copy() if c.clean is not None else None)
        E.check(plain[:, 1].copy(), other, accumulate, "reference", ref=_oracle(O, other, accumulate))
        for j in (0, 2):
            assert _same_bits(got[:, j], plain[:, j]) and _same_bits(plain[:, j], plain[:, 1])


@pytest.mark.parametrize("values", VALUES)
def test_host_tuple_mulV_mulVT_mulM(gpu, pkg, O, values):
    c = E.case("edge", values)
    M = tuple_to_mat(pkg, c.csc())

    def host(case, accumulate):
        return pkg.axpy(M, case.x, case.y0) if accumulate else pkg.mulV(M, case.x)

    _verify(O, host, c, "reference", tree_over=E.STREAM_CHUNK)
    MT = tuple_to_mat(pkg, c.csc_of_transpose())      # (A^T)^T x = A x: the same case through the transposed gather
    _verify(O, lambda case, accumulate: pkg.mulVT(MT, case.x), c, "reference", forms=(False,))
    other = c.clean or c

    def mulm(case, accumulate):
        return pkg.mulM(M, np.stack([other.x, case.x, other.x], axis=1))[:, 1].copy()

    _verify(O, mulm, c, "reference", forms=(False,))
    C = pkg.mulM(M, np.stack([other.x, c.x, other.x], axis=1))
    assert _same_bits(C[:, 0], O.mulV(other.csc(), other.x)) and _same_bits(C[:, 0], C[:, 2])


@pytest.mark.parametrize("values", E.COMPLEX_SETS)
def test_complex_handle(gpu, pkg, O, values):
    """the packed-complex kernel (csrc/spmv_z.hip): poison in the real part, the imaginary part or both; it shares
    the real stream kernel's structure and its documented tree on a row that covers a whole LDS chunk"""
    H = _handle(pkg, "edge", values)
    assert H.is_complex and H.spmv_kernel() == 0
    _verify_handle(gpu, O, H, E.case("edge", values), "reference", tree_over=E.STREAM_CHUNK)


# ---- reference order, the band matrix ---------------------------------------------------------------------------------
@pytest.mark.parametrize("values", VALUES + ("tiny",))
def test_sliced_ell_image(gpu, pkg, O, values):
    """variant 15 on the band: the image is built, and it holds padding (spmv_edge_cases._band asserts both sides)"""
    H = _handle(pkg, "band", values)
    H.set_variant(15)
    assert H.spmv_kernel() == 15 and H.info()["blocked_rows"] == -64
    _verify_handle(gpu, O, H, E.case("band", values), "reference")


# ---- order free, the edge matrix --------------------------------------------------------------------------------------
# (id, form, register sets, environment)
FORMS = [("chunk_k1", "PANEL_FORM_CHUNK_K1", 4, {}), ("chunk_k2", "PANEL_FORM_CHUNK_K2", 4, {}),
         ("paired_k1", "PANEL_FORM_PAIRED_K1", 2, {}), ("paired_k2", "PANEL_FORM_PAIRED_K2", 3, {}),
         ("paired_k2_slices4", "PANEL_FORM_PAIRED_K2", 3, {"SPL_PANEL_SLICES": "4"}),
         ("rounds_u3", "PANEL_FORM_ROUNDS", 3, {}), ("rounds_u5", "PANEL_FORM_ROUNDS", 5, {}),
         ("rounds_free", "PANEL_FORM_ROUNDS", 5, {"SPL_PANEL_RENDEZVOUS": "0"}),
         ("ring_k2", "PANEL_FORM_RING_K2", 0, {})]
SHAPES = [(64, 4), (777, 9)]
TINY_FORMS = ("paired_k2", "rounds_u5")     # tiny: one representative per kernel file
PANEL_CASES = ([f + s + (v,) for f in FORMS for s in SHAPES for v in VALUES]
               + [f + SHAPES[0] + ("tiny",) for f in FORMS if f[0] in TINY_FORMS])


@pytest.mark.parametrize("name,form,unroll,env,P,w,values", PANEL_CASES,
                         ids=["%s-%dx%d-%s" % (c[0], c[4], c[5], c[6]) for c in PANEL_CASES])
def test_panel_forms(gpu, pkg, O, monkeypatch, name, form, unroll, env, P, w, values):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H = _handle(pkg, "edge", values)
    H.build_panel(P, w, unroll, getattr(pkg.DeviceMatrix, form))
    H.set_variant(16)
    assert H.spmv_kernel() == 16 and H.info()["blocked_rows"] == P
    _verify_handle(gpu, O, H, E.case("edge", values), "free")
    assert H.panel_errors() == 0
