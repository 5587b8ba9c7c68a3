"""tests/spmv_edge_cases.py against the oracle alone, no GPU: the oracle passes check() on every value set — in
reference mode against itself, in free mode against the exact row sums — so the reference stays inside every bound and
condition the GPU tests (tests/test_gpu_spmv_edges.py) apply; and check() rejects each defect those tests exist to
catch, applied on the numpy side to the oracle's result."""
import numpy as np
import pytest

import spmv_edge_cases as E

MATRICES = ("edge", "band")


def _oracle(O, c, accumulate):
    A = c.csc()
    if c.is_complex:
        y = c.y0.copy() if accumulate else np.zeros(c.P.nrows, dtype=np.complex128)
        O.axpy_z(A, c.x, y)
        return y
    return O.axpy(A, c.x, c.y0) if accumulate else O.mulV(A, c.x)


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("values", E.REAL_SETS + E.COMPLEX_SETS)
def test_oracle_passes_check(O, matrix, values):
    c = E.case(matrix, values)          # the case module's own conditions are asserted when the case is built
    for accumulate in (False, True):
        y = _oracle(O, c, accumulate)
        clean = _oracle(O, c.clean, accumulate) if c.clean is not None else None
        E.check(y, c, accumulate, "free", clean_got=clean)
        E.check(y.copy(), c, accumulate, "reference", ref=y, clean_got=clean)
        if not c.is_complex:            # the reference order restated in plain Python gives the oracle's bits
            f = E.fold(c, accumulate)
            E.check(f, c, accumulate, "reference", ref=y, clean_got=clean)
            ok = ~np.isnan(y)
            assert np.array_equal(np.signbit(f[ok]), np.signbit(y[ok]))


@pytest.mark.parametrize("values", E.REAL_SETS)
def test_oracle_mulM_passes_check(O, values):
    """three columns of B, the case's x in the middle one: column 1 of C is the case, columns 0 and 2 are the clean x"""
    c = E.case("edge", values)
    other = (c.clean or c).x
    B = np.stack([other, c.x, other], axis=1)
    C = O.mulM(c.csc(), B)
    E.check(C[:, 1].copy(), c, False, "reference", ref=O.mulV(c.csc(), c.x), clean_got=C[:, 0].copy() if c.clean else None)
    assert np.array_equal(C[:, 0], C[:, 2]) and np.array_equal(C[:, 0], O.mulV(c.csc(), other), equal_nan=True)


def test_cases_are_deterministic():
    a = E._build("edge", "poison")
    b = E.case("edge", "poison")
    assert a is not b and np.array_equal(a.vals, b.vals) and np.array_equal(a.x, b.x, equal_nan=True)
    assert np.array_equal(a.P.cols, b.P.cols) and np.array_equal(a.y0, b.y0, equal_nan=True)


# ---- mutants: each must be rejected -----------------------------------------------------------------------------------
def _rejected(got, c, accumulate, mode, ref, **kw):
    with pytest.raises(AssertionError):
        E.check(got, c, accumulate, mode, ref=ref if mode == "reference" else None, **kw)


@pytest.mark.parametrize("mode", ["free", "reference"])
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("column", [0, 16, 512])
def test_mutant_pad_escapes_its_mask(O, matrix, column, mode):
    """0 * x[first column of an index block] added to every row"""
    c = E.case(matrix, "poison")
    for accumulate in (False, True):
        y = _oracle(O, c, accumulate)
        with np.errstate(invalid="ignore"):
            bad = y + 0.0 * c.x[column]
        _rejected(bad, c, accumulate, mode, y)


@pytest.mark.parametrize("mode", ["free", "reference"])
@pytest.mark.parametrize("matrix", MATRICES)
def test_mutant_skips_stored_zeros(O, matrix, mode):
    c = E.case(matrix, "poison")
    for accumulate in (False, True):
        _rejected(E.fold(c, accumulate, skip_zeros=True), c, accumulate, mode, _oracle(O, c, accumulate))


@pytest.mark.parametrize("mode", ["free", "reference"])
@pytest.mark.parametrize("matrix", MATRICES)
def test_mutant_drops_smallest_entry_of_a_cancelling_row(O, matrix, mode):
    c = E.case(matrix, "signed")
    ratio = E.cancellation(c)
    r = int(np.nonzero(np.isfinite(ratio) & (ratio > 2.0 ** 20))[0][7])
    s = c.P.row(r)
    k = int(np.argmin(np.abs(c.vals[s] * c.x[c.P.cols[s]])))
    for accumulate in (False, True):
        _rejected(E.fold(c, accumulate, drop=(r, k)), c, accumulate, mode, _oracle(O, c, accumulate))


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("values", ["signed", "wide"])
def test_mutant_fused_multiply_add(O, matrix, values):
    """a * x + y rounded once is inside the rounding bound (it is the more accurate sum): the bits give it away, so it
    is the reference mode that rejects it"""
    c = E.case(matrix, values)
    for accumulate in (False, True):
        y = _oracle(O, c, accumulate)
        bad = E.fold(c, accumulate, fma=True)
        E.check(bad, c, accumulate, "free")
        _rejected(bad, c, accumulate, "reference", y)


@pytest.mark.parametrize("matrix", ["edge"])          # the band has no empty row
@pytest.mark.parametrize("values", ["signed", "poison"])
def test_mutant_accumulate_starts_from_zero_plus_y0(O, matrix, values):
    """0.0 + (-0.0) is +0.0: free mode compares zeros with ==, reference mode wants the oracle's -0.0 back"""
    c = E.case(matrix, values)
    y = _oracle(O, c, True)
    bad = E.fold(c, True, zero_start=True)
    assert np.sum(np.signbit(y) & (y == 0)) >= 10
    E.check(bad, c, True, "free")
    _rejected(bad, c, True, "reference", y)


@pytest.mark.parametrize("mode", ["free", "reference"])
@pytest.mark.parametrize("matrix", MATRICES)
def test_mutant_flushes_subnormal_products(O, matrix, mode):
    c = E.case(matrix, "tiny")
    for accumulate in (False, True):
        _rejected(E.fold(c, accumulate, flush_products=True), c, accumulate, mode, _oracle(O, c, accumulate))


@pytest.mark.parametrize("mode", ["free", "reference"])
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("values", ["signed", "poison"])
def test_mutant_leaves_rows_unwritten(O, matrix, values, mode):
    """y = A x into a NaN-prefilled y: a kernel that skips rows without entries leaves the prefill there"""
    c = E.case(matrix, values)
    y = _oracle(O, c, False)
    bad = y.copy()
    rows = np.nonzero(c.P.lens == 0)[0] if matrix == "edge" else np.array([50])   # a finite row of the band under poison
    bad[rows] = np.nan
    _rejected(bad, c, False, mode, y)
