"""Inputs and the yardstick of tests/test_gpu_trisolve.py.

The yardstick is the serial loop of include/sparse_linear_hip.h restated on Python floats: every product, difference
and quotient below is one separately rounded IEEE operation (CPython has no fused multiply-add in `a * b - c`), the
complex quotient is the scaled form with math.frexp / math.ldexp, and nothing is summed by numpy.  Everything here runs
on the CPU, so the finiteness of every committed case can be checked without a GPU (`python tests/trisolve_cases.py`).

Inputs keep the solutions bounded: off-diagonal values are uniform in [-1, 1) (each part, when complex), a stored
diagonal has |d_i| >= 1 + sum_j |t_ij| with random signs, and the unit-diagonal variant scales the off-diagonals of every
row so that their absolute sum is at most 0.5."""
import functools
import math

import numpy as np
import scipy.sparse as sp

INF, NAN = float("inf"), float("nan")


# ---- arithmetic ----------------------------------------------------------------------------------------------------
def ieee_div(a, b):
    """a / b as IEEE 754 has it; Python raises on a zero divisor instead"""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def exponent(x):
    """frexp's exponent, 0 for 0 (and for inf / NaN, as math.frexp answers)"""
    return 0 if x == 0.0 else math.frexp(x)[1]


def c_mul(a, b, c, d):
    ac, bd, ad, bc = a * c, b * d, a * d, b * c
    return ac - bd, ad + bc


def c_div(x, y, x1, y1):
    k = -max(exponent(x1), exponent(y1))
    x2, y2 = math.ldexp(x1, k), math.ldexp(y1, k)
    p0, p1 = x1 * x2, y1 * y2
    d = p0 + p1
    a0, a1, b0, b1 = x * x2, y * y2, y * x2, x * y2
    return ieee_div(a0 + a1, d), ieee_div(b0 - b1, d)


# ---- the triangle of a scipy CSR matrix as Python lists ----------------------------------------------------------------
class Triangle(object):
    """rows[i] = (columns, values) of the off-diagonal entries of row i of T, ascending; diag[i] = d_i (0 when no
    diagonal is stored); values are floats, or (re, im) pairs; lower: every column lies below its row"""

    def __init__(self, n, rows, diag, lower, cplx):
        self.n, self.rows, self.diag, self.lower, self.cplx = n, rows, diag, lower, cplx


def take_triangle(S, lower):
    """the Triangle of a scipy matrix S"""
    S = sp.csr_matrix(S)
    S.sort_indices()
    n = S.shape[0]
    cplx = np.iscomplexobj(S.data)
    ptr, idx = S.indptr.tolist(), S.indices.tolist()
    if cplx:
        val = list(zip(S.data.real.tolist(), S.data.imag.tolist()))
    else:
        val = S.data.tolist()
    zero = (0.0, 0.0) if cplx else 0.0
    rows, diag = [], []
    for i in range(n):
        cols, vals, d = [], [], zero
        for q in range(ptr[i], ptr[i + 1]):
            j = idx[q]
            if j == i:
                d = val[q]
            elif (j < i) == lower:
                cols.append(j)
                vals.append(val[q])
        rows.append((cols, vals))
        diag.append(d)
    return Triangle(n, rows, diag, lower, cplx)


def transposed(T, conj):
    """the order-preserving transpose: row j receives (i, t_ij) for ascending i; conjugated first when conj"""
    def cj(v):
        return (v[0], -v[1]) if (conj and T.cplx) else v
    rows = [([], []) for _ in range(T.n)]
    for i in range(T.n):
        cols, vals = T.rows[i]
        for j, v in zip(cols, vals):
            rows[j][0].append(i)
            rows[j][1].append(cj(v))
    return Triangle(T.n, rows, [cj(d) for d in T.diag], not T.lower, T.cplx)


def serial_solve(T, unit, b):
    """one right-hand side b (list of floats or of (re, im) pairs): the loop of the header, row after row"""
    n = T.n
    x = [None] * n
    order = range(n) if T.lower else range(n - 1, -1, -1)
    if not T.cplx:
        for i in order:
            acc = b[i]
            cols, vals = T.rows[i]
            for j, t in zip(cols, vals):
                acc = acc - t * x[j]
            x[i] = acc if unit else ieee_div(acc, T.diag[i])
        return x
    for i in order:
        ar, ai = b[i]
        cols, vals = T.rows[i]
        for j, (tr, ti) in zip(cols, vals):
            xr, xi = x[j]
            pr, pi = c_mul(tr, ti, xr, xi)
            ar, ai = ar - pr, ai - pi
        x[i] = (ar, ai) if unit else c_div(ar, ai, T.diag[i][0], T.diag[i][1])
    return x


def solve_columns(S, lower, unit, op, B):
    """the yardstick for a scipy matrix S and the (n, k) array B: an (n, k) array of the same dtype"""
    T = take_triangle(S, lower)
    if op in ("T", "H"):
        T = transposed(T, op == "H")
    B = np.asarray(B)
    if B.ndim == 1:
        B = B.reshape(-1, 1)
    X = np.empty(B.shape, dtype=np.complex128 if T.cplx else np.float64, order="F")
    for c in range(B.shape[1]):
        if T.cplx:
            col = list(zip(B[:, c].real.tolist(), B[:, c].imag.tolist()))
            x = serial_solve(T, unit, col)
            X[:, c].real = [v[0] for v in x]
            X[:, c].imag = [v[1] for v in x]
        else:
            X[:, c] = serial_solve(T, unit, B[:, c].tolist())
    return X


# ---- patterns: the strictly lower part, (rows, cols) ---------------------------------------------------------------------
def _pattern(name, rng):
    if name == "one":
        return 1, np.zeros(0, int), np.zeros(0, int)
    if name == "diagonal":
        return 300, np.zeros(0, int), np.zeros(0, int)
    if name == "bidiagonal":
        n = 3000
        return n, np.arange(1, n), np.arange(0, n - 1)
    if name in ("dense70", "dense200"):
        n = int(name[5:])
        r, c = np.tril_indices(n, -1)
        return n, r, c
    if name == "poisson":
        m = 40
        i = np.arange(m * m)
        west = i[i % m != 0]
        south = i[i >= m]
        return m * m, np.concatenate([west, south]), np.concatenate([west - 1, south - m])
    if name == "random":
        n = 5000
        want = rng.integers(1, 301, n)  # the row's length, diagonal included
        rows, cols = [], []
        for i in range(n):
            k = min(int(want[i]) - 1, i)
            if k:
                cols.append(rng.choice(i, k, replace=False))
                rows.append(np.full(k, i))
        return n, np.concatenate(rows), np.concatenate(cols)
    if name == "arrow":
        n = 2000
        return n, np.full(n - 1, n - 1), np.arange(n - 1)
    if name == "small":  # for the zero diagonals
        n = 60
        r, c = np.tril_indices(n, -1)
        keep = rng.random(len(r)) < 0.2
        return n, r[keep], c[keep]
    raise KeyError(name)


NAMES = ("one", "diagonal", "bidiagonal", "dense70", "dense200", "poisson", "random", "arrow")
SEEDS = {"one": 11, "diagonal": 12, "bidiagonal": 13, "dense70": 14, "dense200": 15, "poisson": 16, "random": 17,
         "arrow": 18, "small": 19, "full": 20}


def _values(rng, count, cplx):
    v = rng.uniform(-1.0, 1.0, count)
    return v + 1j * rng.uniform(-1.0, 1.0, count) if cplx else v


@functools.lru_cache(maxsize=None)
def matrix(name, cplx, upper=False, unit_scaled=False, with_diag=True):
    """scipy CSR: the lower triangle `name` (its mirror image when upper) with values by the rules above"""
    rng = np.random.default_rng(SEEDS[name] + (100 if cplx else 0))
    n, r, c = _pattern(name, rng)
    v = _values(rng, len(r), cplx)
    rowsum = np.bincount(r, weights=np.abs(v), minlength=n)
    if unit_scaled:
        v = v * (0.5 / np.maximum(rowsum, 0.5))[r]
        rowsum = np.bincount(r, weights=np.abs(v), minlength=n)
    sign = rng.choice([-1.0, 1.0], n)
    d = sign * (1.0 + rowsum)
    if cplx:
        d = d + 0.5j * rng.choice([-1.0, 1.0], n) * (1.0 + rowsum)
    if with_diag:
        r, c, v = np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)]), np.concatenate([v, d])
    S = sp.csr_matrix((v, (r, c)), shape=(n, n))
    if upper:
        S = sp.csr_matrix(S.T)
    S.sort_indices()
    return S


@functools.lru_cache(maxsize=None)
def full_matrix(cplx):
    """an unsymmetric matrix with entries on both sides of a dominant diagonal, n = 400"""
    rng = np.random.default_rng(SEEDS["full"] + (100 if cplx else 0))
    n = 400
    A = sp.random(n, n, density=0.03, random_state=rng, format="coo")
    keep = A.row != A.col
    r, c = A.row[keep], A.col[keep]
    v = _values(rng, len(r), cplx)
    v = v * (0.5 / np.maximum(np.bincount(r, weights=np.abs(v), minlength=n), 0.5))[r]  # fit for a unit diagonal too
    rowsum = np.bincount(r, weights=np.abs(v), minlength=n)
    d = rng.choice([-1.0, 1.0], n) * (1.0 + rowsum)
    if cplx:
        d = d + 0.5j * d
    S = sp.csr_matrix((np.concatenate([v, d]), (np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)]))),
                      shape=(n, n))
    S.sort_indices()
    return S


@functools.lru_cache(maxsize=None)
def rhs(n, k, cplx, seed=5):
    rng = np.random.default_rng(seed * 1000 + n + (7 if cplx else 0))
    B = np.asfortranarray(_values(rng, n * k, cplx).reshape(n, k))
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def reference(name, cplx, upper, unit, op, k):
    """the yardstick's (n, k) result for a committed case; finite, or the case is not fit to be one"""
    S = matrix(name, cplx, upper, unit_scaled=unit)
    X = solve_columns(S, not upper, unit, op, rhs(S.shape[0], k, cplx))
    assert np.all(np.isfinite(X)), (name, cplx, upper, unit, op, k)
    X.setflags(write=False)
    return X


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


if __name__ == "__main__":  # every committed case is finite: checked here, without a GPU
    import time
    for name in NAMES:
        for cplx in (False, True):
            for upper in (False, True):
                for unit in (False, True):
                    for op in "NTH":
                        if name == "random" and (op, unit, upper) not in (("N", False, False), ("T", True, True),
                                                                           ("H", False, False)):
                            continue
                        t0 = time.time()
                        X = reference(name, cplx, upper, unit, op, 1)
                        print("%-10s %-7s %-5s %-6s %s  max |x| %.3g  %.2f s"
                              % (name, "complex" if cplx else "real", "upper" if upper else "lower",
                                 "unit" if unit else "stored", op, float(np.max(np.abs(X))), time.time() - t0))
