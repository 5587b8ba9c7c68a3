"""Inputs and truths for the complex device-handle tests (transpose, ctrans, hermitian, spgemm), built from seeds.

A plain module: no fixtures, no GPU, nothing from the library under test.  Every function takes the CPU oracle `O`
(oracle/oracle.py) and returns oracle CSC tuples (nrows, ncols, pointers, indices, values) or numpy made from them.
tests/test_complex_handle_cases.py checks the properties the GPU tests lean on; tests/test_gpu_complex_handles.py
runs the handles against these truths.

Conventions: a device handle holds the ROW-major image of its matrix, and the CSR arrays of M are the CSC arrays of
M^T; `csr_truth(O, M)` is therefore the oracle's transpose of M, taken on the real and the imaginary parts (the oracle
transposes doubles)."""
import collections

import numpy as np

# rows [row0, row0 + len(rp) - 1) of an nrows_global x ncols matrix as CSR arrays relative to the block
Truth = collections.namedtuple("Truth", "nrows_global ncols row0 rp ci v")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def cplx(re, im):
    """re + i im without arithmetic: the sign bits of zeros survive"""
    v = np.empty(len(re), dtype=np.complex128)
    v.real = re
    v.imag = im
    return v


def from_triples(O, nrows, ncols, r, c, v):
    """CSC tuple of distinct positions (r, c) with values v, real or complex.  The structure comes from O.compress on
    the entry numbers; the values are then moved along that permutation, so no value goes through an addition (which
    would turn -0.0 into +0.0)."""
    r, c, v = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(v)
    assert len(np.unique(r * ncols + c)) == len(r), "positions must be distinct"
    _, _, p, i, pos = O.compress(nrows, ncols, r, c, np.arange(len(r), dtype=np.float64))
    return (nrows, ncols, p, i, np.ascontiguousarray(v[pos.astype(np.int64)]))


def transpose(O, m):
    """O.transpose, on the two parts of a complex tuple"""
    if not np.iscomplexobj(m[4]):
        return O.transpose(m)
    tr = O.transpose(m[:4] + (np.ascontiguousarray(m[4].real),))
    ti = O.transpose(m[:4] + (np.ascontiguousarray(m[4].imag),))
    assert np.array_equal(tr[2], ti[2]) and np.array_equal(tr[3], ti[3])
    return tr[:4] + (cplx(tr[4], ti[4]),)


def ctrans(O, m):
    """omap conj . transpose (Sparse.hs:371-375); np.conj flips the sign bit of the imaginary part, zeros included"""
    t = transpose(O, m)
    return t[:4] + (np.conj(t[4]) if np.iscomplexobj(t[4]) else t[4],)


def csr_truth(O, m):
    """what export_csr of a whole handle of m has to return"""
    t = transpose(O, m)
    return Truth(m[0], m[1], 0, t[2], t[3], t[4])


def rows_of(t, r0, r1):
    """rows [r0, r1) (local numbering) of a truth, as a truth"""
    a, b = int(t.rp[r0]), int(t.rp[r1])
    return Truth(t.nrows_global, t.ncols, t.row0 + r0, t.rp[r0:r1 + 1] - a, t.ci[a:b], t.v[a:b])


def same_matrix(a, b):
    """the derived Eq of Sparse.hs:78 on two tuples: dimensions, pointers, indices, and the values with IEEE =="""
    return bool(a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
                and np.array_equal(a[4], b[4]))


def hermitian_by_definition(O, m):
    """hermitian m = ctrans m == m (Sparse.hs:377-379)"""
    return same_matrix(ctrans(O, m), m)


def sensitive(rng, k):
    """values spread over seven decades: sums of their products depend on the order"""
    return rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, k)


def sensitive_z(rng, k):
    im = sensitive(rng, k)
    im[im == 0.0] = 1.0
    return cplx(sensitive(rng, k), im)


# ---- transpose / ctrans -----------------------------------------------------------------------------------------

T_NR, T_NC = 5003, 1201
T_EMPTY_ROWS = (0, 1, 2, T_NR - 2, T_NR - 1)
T_EMPTY_COLS = (0, 600, T_NC - 1)
T_SINGLE_COLS = (1, 601)
T_LONG_COL, T_LONG_LEN = 700, 4200     # beyond the 4096 entries the segmented sort keeps in LDS
T_MID_COL, T_MID_LEN = 333, 300        # one workgroup, sorted in LDS


def transpose_input(O):
    """5003 x 1201 complex, about 20 000 entries: the columns — the segments the device transpose sorts — have 0, 1,
    2 to 64, 300 and 4 200 entries; rows are empty at both ends; a few imaginary parts are +0.0 and -0.0"""
    rng = np.random.default_rng(5003_1201)
    usable = np.setdiff1d(np.arange(T_NR), T_EMPTY_ROWS)
    r, c = [], []
    for j in range(T_NC):
        if j in T_EMPTY_COLS:
            n = 0
        elif j in T_SINGLE_COLS:
            n = 1
        elif j == T_LONG_COL:
            n = T_LONG_LEN
        elif j == T_MID_COL:
            n = T_MID_LEN
        else:
            n = 64 if j == 2 else 2 if j == 3 else int(rng.integers(2, 25))
        r.append(rng.choice(usable, n, replace=False))
        c.append(np.full(n, j))
    r, c = np.concatenate(r), np.concatenate(c)
    v = sensitive_z(rng, len(r))
    zeros = rng.choice(len(r), 8, replace=False)
    v[zeros[:4]] = cplx(v[zeros[:4]].real, np.full(4, 0.0))
    v[zeros[4:]] = cplx(v[zeros[4:]].real, np.full(4, -0.0))
    order = rng.permutation(len(r))
    return from_triples(O, T_NR, T_NC, r[order], c[order], v[order])


def small_inputs(O):
    """the 1 x 1 and a 37 x 129 complex matrix"""
    rng = np.random.default_rng(37_129)
    one = from_triples(O, 1, 1, [0], [0], np.array([2.5 - 0.75j]))
    key = np.unique(rng.integers(0, 37 * 129, 900))
    small = from_triples(O, 37, 129, key // 129, key % 129, sensitive_z(rng, len(key)))
    return {"1x1": one, "37x129": small}


def real_part(m):
    return m[:4] + (np.ascontiguousarray(m[4].real),)


# ---- hermitian --------------------------------------------------------------------------------------------------

H_N = 1500
H_ARROW, H_ARROW_LEN = 1400, 300


def _hermitian_triples(rng):
    """A = L + L^H + real diagonal as triples: L strictly lower, about 12 000 entries, row H_ARROW with 300"""
    key = np.unique(rng.integers(0, H_N, 25_000) * H_N + rng.integers(0, H_N, 25_000))
    i, j = key // H_N, key % H_N
    keep = (i > j) & (i != H_ARROW) & (j != H_ARROW)
    i, j = i[keep], j[keep]
    i = np.concatenate([i, np.full(H_ARROW_LEN, H_ARROW)])
    j = np.concatenate([j, rng.choice(H_ARROW, H_ARROW_LEN, replace=False)])
    lv = sensitive_z(rng, len(i))
    d = np.arange(H_N)
    r = np.concatenate([i, j, d])
    c = np.concatenate([j, i, d])
    v = np.concatenate([lv, np.conj(lv), sensitive(rng, H_N) + 0j])
    return r, c, v, len(i)


def hermitian_cases(O):
    """name -> (CSC tuple, complex?) for every row of the issue's table; the verdicts are hermitian_by_definition's"""
    rng = np.random.default_rng(1500)
    r, c, v, nl = _hermitian_triples(rng)
    cases = {}

    def put(name, r_, c_, v_, n=H_N, m=H_N):
        cases[name] = from_triples(O, n, m, r_, c_, v_)

    put("A", r, c, v)
    k = 17                                    # an entry of L; its mirror is entry nl + k
    w = v.copy()
    w[k] = complex(w[k].real, np.nextafter(w[k].imag, np.inf))
    put("imag_one_ulp", r, c, w)
    w = v.copy()
    w[2 * nl + 700] = complex(w[2 * nl + 700].real, 1e-300)
    put("diagonal_imag_1e-300", r, c, w)
    w = v.copy()
    w[nl + k] = 3.0 - 4.0j
    put("one_side_replaced", r, c, w)
    have = set((r * H_N + c).tolist())
    i0, j0 = next((a, b) for a in range(900, H_N) for b in range(10, a)
                  if a * H_N + b not in have and b * H_N + a not in have)
    put("stored_zero_without_mirror", np.append(r, i0), np.append(c, j0), np.append(v, 0j))
    w = v.copy()
    w[k] = cplx([0.0], [-0.0])[0]
    w[nl + k] = cplx([-0.0], [-0.0])[0]
    put("signed_zero_pair", r, c, w)
    w = v.copy()
    w[2 * nl + 3] = complex(np.nan, 0.0)
    put("nan_on_diagonal", r, c, w)
    put("real_symmetric", r, c, np.ascontiguousarray(v.real))
    w = np.ascontiguousarray(v.real)
    w[nl + k] = np.nextafter(w[nl + k], np.inf)
    put("real_asymmetric", r, c, w)
    none = np.zeros(0, dtype=np.int64)
    put("no_entries", none, none, np.zeros(0, dtype=np.complex128))
    put("no_entries_real", none, none, np.zeros(0))
    keep = c < H_N - 1
    put("not_square", r[keep], c[keep], v[keep], H_N, H_N - 1)
    return cases


# the issue's table; "real_symmetric_to_complex" is real_symmetric promoted on the device
H_EXPECTED = {"A": True, "imag_one_ulp": False, "diagonal_imag_1e-300": False, "one_side_replaced": False,
              "stored_zero_without_mirror": False, "signed_zero_pair": True, "nan_on_diagonal": False,
              "real_symmetric": True, "real_asymmetric": False, "no_entries": True, "no_entries_real": True,
              "not_square": False}


# ---- spgemm -----------------------------------------------------------------------------------------------------

G_NR, G_NK, G_NC = 300, 400, 2000
G_EMPTY_ROWS = (0, 1, 150, G_NR - 1)
G_HEAVY_ROW, G_HEAVY_LEN = 200, 70       # its row of A B has more than 1 024 entries
G_BLOCK = (37, 211)                      # a row block of A whose cut is no multiple of 64; holds the heavy row
G_ALPHA, G_BETA = 0.75 - 1.25j, -0.5 + 2.0j


def _left_pattern(rng):
    r, c = [], []
    for i in range(G_NR):
        n = 0 if i in G_EMPTY_ROWS else G_HEAVY_LEN if i == G_HEAVY_ROW else int(rng.integers(1, 20))
        r.append(np.full(n, i))
        c.append(rng.choice(G_NK, n, replace=False))
    return np.concatenate(r), np.concatenate(c)


def spgemm_inputs(O):
    """A 300 x 400 and B 400 x 2000 complex, about 3 000 and 24 000 entries; R1, R2 real 300 x 400 with different
    patterns, from which the GPU test makes the second left factor A2 = R1 + 0.5j R2 on the device"""
    rng = np.random.default_rng(300_400_2000)
    r, c = _left_pattern(rng)
    A = from_triples(O, G_NR, G_NK, r, c, sensitive_z(rng, len(r)))
    key = np.unique(rng.integers(0, G_NK * G_NC, 24_400))
    B = from_triples(O, G_NK, G_NC, key // G_NC, key % G_NC, sensitive_z(rng, len(key)))
    r1, c1 = _left_pattern(rng)
    R1 = from_triples(O, G_NR, G_NK, r1, c1, sensitive(rng, len(r1)))
    r2, c2 = _left_pattern(rng)
    R2 = from_triples(O, G_NR, G_NK, r2, c2, sensitive(rng, len(r2)))
    return {"A": A, "B": B, "R1": R1, "R2": R2}


def spgemm_truths(O, inp):
    """oracle results: A2 = lin_z(1, R1, 0.5j, R2), AB = mm_z(A, B), A2B = mm_z(A2, B),
    lin = lin_z(alpha, AB, beta, A2B)"""
    A2 = O.lin_z(1.0, inp["R1"], 0.5j, inp["R2"])
    AB = O.mm_z(inp["A"], inp["B"])
    A2B = O.mm_z(A2, inp["B"])
    return {"A2": A2, "AB": AB, "A2B": A2B, "lin": O.lin_z(G_ALPHA, AB, G_BETA, A2B)}
