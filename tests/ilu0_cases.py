"""Inputs and the yardstick of tests/test_gpu_ilu0.py and tests/test_ilu0_cpu.py.

The yardstick is the serial IKJ loop of include/sparse_linear_hip.h restated on Python floats:

    for i:  for each stored (i,k), k < i, ascending:   a_ik = a_ik / u_kk        (u_kk = 0 when row k stores none)
                for each stored (i,j), j > k:           if (k,j) is stored:  a_ij = a_ij - a_ik * a_kj

Every product, difference and quotient is one separately rounded IEEE operation (CPython has no fused multiply-add in
`a - l * b`); the division, the complex product and the scaled complex quotient are those of tests/trisolve_cases.py
(ieee_div, c_mul, c_div).  Nothing is summed by numpy.  Inside one step k the entries (i,j) are independent of each
other, so the loop may visit them in any order: it walks the shorter of the two runs and looks the column up in the other.

Inputs: off-diagonal values uniform in [-1, 1) (each part, when complex), diagonal |d_i| >= 1 + sum_j |a_ij| with random
signs, so every committed case stays finite (`python tests/ilu0_cases.py` checks that on the CPU) — except the two that
are meant not to be: "strictlower" (no row stores a diagonal) and "pivots" (a stored zero and a missing diagonal)."""
import functools
import math

import numpy as np
import scipy.sparse as sp

from trisolve_cases import c_div, c_mul, ieee_div

NAMES = ("poisson40", "poisson32", "tridiagonal", "dense70", "arrow", "blocks", "identity", "strictlower", "random")
SEEDS = {name: 31 + i for i, name in enumerate(NAMES + ("pivots",))}
SIZES = {"poisson40": 40, "poisson32": 32, "tridiagonal": 3000, "dense70": 70, "arrow": 500, "blocks": 300,
         "identity": 300, "strictlower": 400, "random": 600, "pivots": 60}


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def serial_ilu0(S, count=None):
    """the L\\U values of the scipy CSR matrix S (sorted indices, explicit zeros are entries) in S's own entry order:
    a float64 or complex128 array.  count: a list that receives the number of inner updates"""
    S = sp.csr_matrix(S)
    assert S.has_sorted_indices
    n = S.shape[0]
    cplx = np.iscomplexobj(S.data)
    ptr, idx = S.indptr.tolist(), S.indices.tolist()
    val = list(zip(S.data.real.tolist(), S.data.imag.tolist())) if cplx else S.data.tolist()
    zero = (0.0, 0.0) if cplx else 0.0
    diag = [-1] * n    # position of the stored a_ii
    above = [None] * n  # row k: {j: position} over its entries with j > k
    updates = 0
    for i in range(n):
        s, e = ptr[i], ptr[i + 1]
        mine = {idx[t]: t for t in range(s, e)}
        for q in range(s, e):
            k = idx[q]
            if k >= i:
                break
            u = val[diag[k]] if diag[k] >= 0 else zero
            if cplx:
                l = c_div(val[q][0], val[q][1], u[0], u[1])
            else:
                l = ieee_div(val[q], u)
            val[q] = l
            theirs = above[k]
            if len(theirs) <= e - q - 1:
                pairs = [(mine[j], r) for j, r in theirs.items() if j in mine]
            else:
                pairs = [(t, theirs[idx[t]]) for t in range(q + 1, e) if idx[t] in theirs]
            updates += len(pairs)
            if cplx:
                for t, r in pairs:
                    pr, pi = c_mul(l[0], l[1], val[r][0], val[r][1])
                    val[t] = (val[t][0] - pr, val[t][1] - pi)
            else:
                for t, r in pairs:
                    val[t] = val[t] - l * val[r]
        above[i] = {idx[t]: t for t in range(s, e) if idx[t] > i}
        if i in mine:
            diag[i] = mine[i]
    if count is not None:
        count.append(updates)
    if cplx:
        out = np.empty(len(val), dtype=np.complex128)
        out.real = [v[0] for v in val]
        out.imag = [v[1] for v in val]
        return out
    return np.array(val, dtype=np.float64)


# ---- patterns: the off-diagonal entries, (rows, cols), and whether a diagonal is stored --------------------------------
def _random_lengths(rng, n):
    """stored entries of every row, diagonal included: 1 ... 300, every power-of-two class and rows of several chunks
    of 64 among them (asserted by groups_of_rows below); row 0 stores its diagonal alone"""
    want = np.floor(2.0 ** rng.uniform(1.0, math.log2(301.0), n)).astype(int).clip(2, 300)
    want[0] = 1
    want[1:8] = (2, 3, 5, 300, 129, 64, 65)
    return want


def _pattern(name, n, rng):
    none = np.zeros(0, int)
    if name in ("poisson40", "poisson32"):
        m = n
        i = np.arange(m * m)
        west, east, south, north = i[i % m != 0], i[i % m != m - 1], i[i >= m], i[i < m * m - m]
        return (m * m, np.concatenate([west, east, south, north]),
                np.concatenate([west - 1, east + 1, south - m, north + m]), True)
    if name == "tridiagonal":
        return n, np.concatenate([np.arange(1, n), np.arange(0, n - 1)]), np.concatenate([np.arange(0, n - 1), np.arange(1, n)]), True
    if name == "dense70":
        r, c = np.nonzero(~np.eye(n, dtype=bool))
        return n, r, c, True
    if name == "arrow":  # full last row and last column: pointing down-right, no fill
        a = np.arange(n - 1)
        return n, np.concatenate([np.full(n - 1, n - 1), a]), np.concatenate([a, np.full(n - 1, n - 1)]), True
    if name == "blocks":  # n independent dense 3 x 3 blocks
        b = 3 * np.repeat(np.arange(n), 6)
        r = np.tile(np.array([0, 0, 1, 1, 2, 2]), n)
        c = np.tile(np.array([1, 2, 0, 2, 0, 1]), n)
        return 3 * n, b + r, b + c, True
    if name == "identity":
        return n, none, none, True
    if name == "strictlower":
        r, c = np.tril_indices(n, -1)
        keep = rng.random(len(r)) < 0.02
        return n, r[keep], c[keep], False
    if name == "random":
        want = _random_lengths(rng, n)
        rows, cols = [], []
        for i in range(n):
            fixed = [i - 1] if i > 0 and want[i] > 1 else []  # the row above: level(i) = i, one row per level
            others = np.setdiff1d(np.arange(n), [i] + fixed)
            pick = rng.choice(others, int(want[i]) - 1 - len(fixed), replace=False)
            cols.append(np.concatenate([np.array(fixed, int), pick]))
            rows.append(np.full(len(cols[-1]), i))
        return n, np.concatenate(rows), np.concatenate(cols), True
    if name == "pivots":
        r, c = np.nonzero(~np.eye(n, dtype=bool))
        keep = rng.random(len(r)) < 0.2
        keep &= ~((r == 5) & (c < 5))  # row 5 has no lower part: its stored diagonal is its final u
        r, c = r[keep], c[keep]
        extra = [(20, 5), (41, 5), (30, 12), (50, 12), (12, 3)]  # dependants of rows 5 and 12; row 12 has a lower part
        have = set(zip(r.tolist(), c.tolist()))
        extra = [p for p in extra if p not in have]
        return (n, np.concatenate([r, np.array([p[0] for p in extra], int)]),
                np.concatenate([c, np.array([p[1] for p in extra], int)]), True)
    raise KeyError(name)


def _values(rng, count, cplx):
    v = rng.uniform(-1.0, 1.0, count)
    return v + 1j * rng.uniform(-1.0, 1.0, count) if cplx else v


@functools.lru_cache(maxsize=None)
def matrix(name, cplx, size=None, values=0):
    """scipy CSR with sorted indices: the pattern `name` (SIZES[name], or `size`) with values by the rules above;
    values = 1, 2 ...: other values on the same pattern"""
    n0 = SIZES[name] if size is None else size
    n, r, c, with_diag = _pattern(name, n0, np.random.default_rng(SEEDS[name]))
    rng = np.random.default_rng(SEEDS[name] + (100 if cplx else 0) + 1000 * values)
    v = _values(rng, len(r), cplx)
    rowsum = np.bincount(r, weights=np.abs(v), minlength=n)
    d = rng.choice([-1.0, 1.0], n) * (1.0 + rowsum)
    if cplx:
        d = d + 0.5j * rng.choice([-1.0, 1.0], n) * (1.0 + rowsum)
    if with_diag:
        r, c, v = np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)]), np.concatenate([v, d])
    S = sp.csr_matrix((v, (r, c)), shape=(n, n))
    S.sort_indices()
    assert S.nnz == len(v)  # no duplicates were summed
    return S


@functools.lru_cache(maxsize=None)
def laplacian(m):
    """the 5-point Laplacian on an m x m grid, 4 on and -1 beside the diagonal: weakly dominant, so an iteration
    preconditioned by its ILU(0) converges at a rate that shows (the dominant random values converge in a few steps)"""
    n, r, c, _ = _pattern("poisson32", m, None)
    r, c = np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)])
    S = sp.csr_matrix((np.where(r == c, 4.0, -1.0), (r, c)), shape=(n, n))
    S.sort_indices()
    return S


@functools.lru_cache(maxsize=None)
def pivots_cases(cplx):
    """(both, zero, good).  Row 5 has no lower part, so its stored diagonal is its final u; rows 5 and 12 have
    dependants.  both: row 5 stores a 0.0 diagonal and row 12 stores none.  zero and good share the full pattern (every
    diagonal stored): zero has the 0.0 in row 5, good has the dominant diagonal everywhere.  A pattern without (12, 12)
    is singular whatever its values are, so "the same pattern with good values" is asked of the full pattern"""
    good = sp.csr_matrix(matrix("pivots", cplx))
    full = sp.coo_matrix(good)
    n = full.shape[0]
    v0 = full.data.copy()
    v0[(full.row == 5) & (full.col == 5)] = 0.0
    zero = sp.csr_matrix((v0, (full.row, full.col)), shape=(n, n))  # (explicit zeros stay entries)
    keep = ~((full.row == 12) & (full.col == 12))
    both = sp.csr_matrix((v0[keep], (full.row[keep], full.col[keep])), shape=(n, n))
    for S, nnz in ((zero, good.nnz), (both, good.nnz - 1)):
        S.sort_indices()
        assert S.nnz == nnz
    return both, zero, good


@functools.lru_cache(maxsize=None)
def reference(name, cplx, size=None, values=0):
    """the yardstick's values for a committed case, in the entry order of matrix(...); finite unless the case says no"""
    S = matrix(name, cplx, size, values)
    count = []
    out = serial_ilu0(S, count)
    assert count[0] <= 2000000, (name, count[0])
    if name != "strictlower":
        assert np.all(np.isfinite(out.view(np.float64))), (name, cplx)
    out.setflags(write=False)
    return out


def factors_of(S, values):
    """(L, U) as scipy CSR matrices from L\\U values in S's entry order: L unit lower, U upper with the diagonal"""
    F = sp.csr_matrix((np.asarray(values), S.indices, S.indptr), shape=S.shape)
    L = sp.tril(F, -1, format="csr") + sp.identity(S.shape[0], dtype=F.dtype, format="csr")
    return sp.csr_matrix(L), sp.triu(F, 0, format="csr")


def groups_of_rows(S):
    """the lanes per row the launch plan picks when every row is a level of its own: the power of two >= the row's
    length, 1 ... 64"""
    out = set()
    for length in np.diff(S.indptr).tolist():
        g = 1
        while g < 64 and g < length:
            g <<= 1
        out.add(g)
    return out


def levels_of(S):
    """level(i) = 1 + max level(k) over the stored (i,k) with k < i; the number of levels"""
    S = sp.csr_matrix(S)
    ptr, idx = S.indptr.tolist(), S.indices.tolist()
    level = [0] * S.shape[0]
    for i in range(S.shape[0]):
        below = [level[k] + 1 for k in idx[ptr[i]:ptr[i + 1]] if k < i]
        level[i] = max(below) if below else 0
    return level


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def nan_or_bits_equal(a, b):
    a = np.ascontiguousarray(a).view(np.float64)
    b = np.ascontiguousarray(b).view(np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


if __name__ == "__main__":  # every committed case is finite and small enough: checked here, without a GPU
    import time
    for name in NAMES:
        for cplx in (False, True):
            t0 = time.time()
            S = matrix(name, cplx)
            count = []
            out = serial_ilu0(S, count)
            finite = bool(np.all(np.isfinite(out.view(np.float64))))
            assert finite == (name != "strictlower"), name
            print("%-12s %-7s n %5d nnz %6d longest row %3d levels %4d updates %7d finite %-5s max |f| %.3g  %.2f s"
                  % (name, "complex" if cplx else "real", S.shape[0], S.nnz, int(np.diff(S.indptr).max()),
                     max(levels_of(S)) + 1, count[0], finite,
                     float(np.max(np.abs(out[np.isfinite(out)]), initial=0.0)), time.time() - t0))
    assert groups_of_rows(matrix("random", False)) == {1, 2, 4, 8, 16, 32, 64}
    assert levels_of(matrix("random", False)) == list(range(600))
    for cplx in (False, True):
        both, zero, good = pivots_cases(cplx)
        assert not np.all(np.isfinite(serial_ilu0(both).view(np.float64)))
        assert not np.all(np.isfinite(serial_ilu0(zero).view(np.float64)))
        assert np.all(np.isfinite(serial_ilu0(good).view(np.float64)))
