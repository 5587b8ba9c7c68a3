"""The inputs of tests/test_gpu_complex_handles.py have the properties those tests lean on (no GPU, oracle only):
the segment lengths that reach every regime of the device's segmented sort, the Hermitian verdicts by definition,
and the row lengths of the complex product that reach every path of its value kernel."""
import numpy as np
import pytest

import complex_handle_cases as K


@pytest.fixture(scope="module")
def tin(O):
    return K.transpose_input(O)


def test_transpose_input_reaches_every_sort_regime(O, tin):
    nr, nc, p, i, v = tin
    assert (nr, nc) == (K.T_NR, K.T_NC) and 19_000 < len(i) < 21_000
    assert O.check_matrix(K.real_part(tin)) == 0
    cols = np.diff(p)
    assert all(cols[j] == 0 for j in K.T_EMPTY_COLS) and all(cols[j] == 1 for j in K.T_SINGLE_COLS)
    assert cols[2] == 64 and cols[3] == 2                       # the ends of the one-wavefront regime
    assert cols[K.T_MID_COL] == K.T_MID_LEN and 64 < K.T_MID_LEN <= 4096
    assert cols[K.T_LONG_COL] == K.T_LONG_LEN > 4096            # sorted in global memory
    others = np.delete(cols, list(K.T_EMPTY_COLS + K.T_SINGLE_COLS) + [K.T_MID_COL, K.T_LONG_COL])
    assert others.min() >= 2 and others.max() <= 64
    rows = np.bincount(i, minlength=nr)
    assert all(rows[r] == 0 for r in K.T_EMPTY_ROWS)
    # rounding-sensitive values with imaginary parts, a few of them zeros of either sign
    im = v.imag
    assert np.count_nonzero((im == 0) & ~np.signbit(im)) == 4 and np.count_nonzero((im == 0) & np.signbit(im)) == 4
    assert np.count_nonzero(im) == len(im) - 8 and not np.array_equal(v.real, np.round(v.real))


def test_oracle_transposes_invert_each_other(O, tin):
    """transpose . transpose = id and ctrans . ctrans = id bit for bit, conj flips the sign bit of zeros"""
    for m in [tin] + list(K.small_inputs(O).values()):
        for f in (K.transpose, K.ctrans):
            back = f(O, f(O, m))
            assert back[:2] == m[:2] and np.array_equal(back[2], m[2]) and np.array_equal(back[3], m[3])
            assert K.same_bits(back[4], m[4])
    t, ct = K.transpose(O, tin), K.ctrans(O, tin)
    assert K.same_bits(t[4].real, ct[4].real)
    assert np.array_equal(np.signbit(t[4].imag), ~np.signbit(ct[4].imag))
    # the CSR arrays of A^T are the CSC arrays of A
    tt = K.csr_truth(O, t)
    assert np.array_equal(tt.rp, tin[2]) and np.array_equal(tt.ci, tin[3]) and K.same_bits(tt.v, tin[4])


def test_small_inputs(O):
    s = K.small_inputs(O)
    assert s["1x1"][:2] == (1, 1) and len(s["1x1"][3]) == 1
    assert s["37x129"][:2] == (37, 129) and len(s["37x129"][3]) > 500


@pytest.fixture(scope="module")
def hcases(O):
    return K.hermitian_cases(O)


def test_hermitian_base_matrix(O, hcases):
    n, m, p, i, v = hcases["A"]
    assert n == m == K.H_N and 24_000 < len(i) < 28_000
    cols = np.diff(p)
    assert cols[K.H_ARROW] == K.H_ARROW_LEN + 1 > 64            # the arrow row and, mirrored, the arrow column
    rows = np.bincount(i, minlength=n)
    assert rows[K.H_ARROW] == K.H_ARROW_LEN + 1
    assert np.count_nonzero(v.imag) > 24_000 - K.H_N
    assert hcases["not_square"][:2] == (K.H_N, K.H_N - 1)
    assert len(hcases["no_entries"][3]) == 0 and hcases["no_entries"][:2] == (K.H_N, K.H_N)
    assert len(hcases["stored_zero_without_mirror"][3]) == len(i) + 1
    assert not np.iscomplexobj(hcases["real_symmetric"][4]) and not np.iscomplexobj(hcases["real_asymmetric"][4])


def test_hermitian_verdicts_by_definition(O, hcases):
    assert set(hcases) == set(K.H_EXPECTED)
    for name, m in hcases.items():
        assert K.hermitian_by_definition(O, m) == K.H_EXPECTED[name], name
    # the promoted real symmetric matrix: conj makes its +0.0 imaginary parts -0.0, and == does not mind
    s = hcases["real_symmetric"]
    z = s[:4] + (K.cplx(s[4], np.zeros(len(s[4]))),)
    assert K.hermitian_by_definition(O, z)
    assert np.all(np.signbit(K.ctrans(O, z)[4].imag)) and not np.any(np.signbit(z[4].imag))
    # the pattern cases differ from A in exactly what their names say
    A = hcases["A"]
    for name in ("imag_one_ulp", "diagonal_imag_1e-300", "one_side_replaced", "signed_zero_pair", "nan_on_diagonal"):
        m = hcases[name]
        assert np.array_equal(m[2], A[2]) and np.array_equal(m[3], A[3])
        assert 1 <= np.count_nonzero(K.bits(m[4]).reshape(-1, 2) != K.bits(A[4]).reshape(-1, 2)) <= 4, name


def test_spgemm_inputs_reach_every_path_of_the_value_kernel(O):
    inp = K.spgemm_inputs(O)
    A, B = inp["A"], inp["B"]
    assert A[:2] == (K.G_NR, K.G_NK) and B[:2] == (K.G_NK, K.G_NC)
    assert 2_700 < len(A[3]) < 3_300 and 23_000 < len(B[3]) < 25_000
    assert np.count_nonzero(A[4].imag) == len(A[4]) and np.count_nonzero(B[4].imag) == len(B[4])
    t = K.spgemm_truths(O, inp)
    for name in ("AB", "A2B"):
        C = t[name]
        assert C[:2] == (K.G_NR, K.G_NC)
        rows = np.bincount(C[3], minlength=K.G_NR)   # the handle holds rows: the kernel cuts ROWS into 512-entry chunks
        assert all(rows[r] == 0 for r in K.G_EMPTY_ROWS)
        assert rows[K.G_HEAVY_ROW] > 1024            # three chunks, and the bisection into A's slices
        assert np.count_nonzero((rows > 0) & (rows <= 512)) > 10 and np.count_nonzero((rows > 512) & (rows <= 1024)) > 10
    r0, r1 = K.G_BLOCK
    assert r0 % 64 and r1 % 64 and r0 < K.G_HEAVY_ROW < r1 and r0 < 150 < r1
    # A2's pattern is the union of two different ones
    assert len(t["A2"][3]) > max(len(inp["R1"][3]), len(inp["R2"][3]))
    assert not np.array_equal(inp["R1"][3], inp["R2"][3])
