"""The yardstick of tests/test_gpu_first_walk.py, checked without a GPU: helpers.exact_backward_error against rational
arithmetic, and the reference's own raw walk on every input of tests/first_walk_cases.py."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import first_walk_cases as F
from helpers import exact_backward_error, real_embedding, two_product


def rational_backward_error(S, x, b):
    """the same quantity in exact rational arithmetic on a dense real matrix, rounded once at the end"""
    S = np.asarray(S, dtype=np.float64)
    worst = Fraction(0)
    for i in range(S.shape[0]):
        r = Fraction(float(b[i])) - sum((Fraction(float(S[i, j])) * Fraction(float(x[j])) for j in range(S.shape[1])),
                                        Fraction(0))
        den = abs(Fraction(float(b[i]))) + sum((abs(Fraction(float(S[i, j])) * Fraction(float(x[j])))
                                                for j in range(S.shape[1])), Fraction(0))
        if r == 0:
            continue
        if den == 0:
            return float("inf")
        worst = max(worst, abs(r) / den)
    return float(worst)


def dense_embedding(S):
    n = S.shape[0]
    E = np.zeros((2 * n, 2 * n))
    E[0::2, 0::2], E[0::2, 1::2], E[1::2, 0::2], E[1::2, 1::2] = S.real, -S.imag, S.imag, S.real
    return E


def close(a, b):
    # the helper rounds |r_i|, the denominator and their quotient once each; the rational value is rounded once
    return a == b or abs(a - b) <= 4 * 2.0 ** -53 * abs(b)


def test_two_product_is_exact():
    rng = np.random.default_rng(1)
    a = rng.normal(size=2000) * 10.0 ** rng.integers(-8, 9, 2000)
    b = rng.normal(size=2000) * 10.0 ** rng.integers(-8, 9, 2000)
    p, e = two_product(a, b)
    for ai, bi, pi, ei in zip(a.tolist(), b.tolist(), p.tolist(), e.tolist()):
        assert Fraction(ai) * Fraction(bi) == Fraction(pi) + Fraction(ei)


@pytest.mark.parametrize("seed", range(6))
def test_helper_against_rational_arithmetic_real(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 30))
    S = rng.normal(size=(n, n)) * (rng.random((n, n)) < 0.5) + np.diag(rng.uniform(1.0, 2.0, n) * n)
    xs = rng.uniform(0.5, 1.5, n)
    b = S @ xs
    x = np.linalg.solve(S, b)
    for cand in (x, xs, np.nextafter(x, np.inf) * (np.arange(n) == n // 2) + x * (np.arange(n) != n // 2)):
        w = exact_backward_error(sp.csr_matrix(S), cand, b)
        assert close(w, rational_backward_error(S, cand, b)), seed
        assert exact_backward_error(sp.csc_matrix(S), cand, b) == w  # the storage order of the entries does not matter


@pytest.mark.parametrize("seed", range(4))
def test_helper_against_rational_arithmetic_complex(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 16))
    S = (rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))) * (rng.random((n, n)) < 0.6) \
        + np.diag((3.0 + 0.5j) * n * np.ones(n))
    xs = rng.uniform(0.5, 1.5, n) + 1j * rng.uniform(-1.0, 1.0, n)
    b = S @ xs
    x = np.linalg.solve(S, b)
    E = dense_embedding(S)
    assert np.array_equal(real_embedding(sp.csr_matrix(S)).toarray(), E)
    for cand in (x, xs):
        w = exact_backward_error(sp.csr_matrix(S), cand, b)
        assert close(w, rational_backward_error(E, cand.view(np.float64), b.view(np.float64))), seed
    # the ordering of the pairs does not matter: the rows of the embedding with (re, im) exchanged give the same figure
    q = np.arange(2 * n).reshape(n, 2)[:, ::-1].ravel()
    assert close(rational_backward_error(E[q], x.view(np.float64), b.view(np.float64)[q]), exact_backward_error(S, x, b))


def test_helper_with_heavy_cancellation_and_one_ulp():
    """rows whose products cancel to the last bits: a plain S @ x - b is wrong in its leading digit there"""
    rng = np.random.default_rng(5)
    n = 12
    S = np.zeros((n, n))
    for i in range(n):
        j = (i + 1) % n
        S[i, i], S[i, j] = 1e8 + rng.random(), -(1e8 + rng.random())
        S[i, (i + 5) % n] = rng.random()
    x = 1.0 + rng.random(n) * 1e-9
    b = S @ x
    for cand in (x, np.where(np.arange(n) == 3, np.nextafter(x, 2.0), x)):
        assert close(exact_backward_error(sp.csr_matrix(S), cand, b), rational_backward_error(S, cand, b))
    one_ulp = exact_backward_error(sp.csr_matrix(S), np.where(np.arange(n) == 3, np.nextafter(x, 2.0), x), b)
    assert 0.0 < one_ulp < 2.0 ** -52


def test_helper_on_exact_integer_data_returns_zero():
    rng = np.random.default_rng(9)
    S = sp.random(40, 40, density=0.2, random_state=rng, format="csr")
    S.data = np.round(S.data * 50.0) + 1.0
    S = S + sp.identity(40) * 300.0
    x = rng.integers(-50, 51, 40).astype(float)
    b = S @ x
    assert exact_backward_error(S, x, b) == 0.0
    Z = sp.csr_matrix(S + 1j * sp.identity(40) * 7.0)
    z = x + 1j * rng.integers(-50, 51, 40)
    assert exact_backward_error(Z, z, Z @ z) == 0.0
    ws = exact_backward_error(S, [x, x + 1.0], [b, b])
    assert ws[0] == 0.0 and ws[1] > 0.0


def test_helper_zero_denominator_and_batches():
    S = sp.csr_matrix(np.array([[0.0, 0.0], [0.0, 2.0]]))
    assert exact_backward_error(S, np.array([1.0, 1.0]), np.array([0.0, 2.0])) == 0.0  # 0 / 0 counts as no error
    S = sp.csr_matrix(np.array([[1.0, 0.0], [0.0, 2.0]]))
    assert exact_backward_error(S, np.array([0.0, 1.0]), np.array([0.0, 2.0])) == 0.0
    assert exact_backward_error(S, np.array([1.0, 1.0]), np.array([0.0, 2.0])) == 1.0
    # a residual over a zero denominator: only possible with a stored zero row and b_i != 0 after underflow; inf and
    # NaN in the solution count as the worst
    assert exact_backward_error(S, np.array([np.nan, 1.0]), np.array([1.0, 2.0])) == math.inf
    ws = exact_backward_error(S, np.array([[1.0, 1.0], [0.5, 1.0], [1.0, 0.5]]), np.array([[1.0, 2.0]] * 3))
    assert isinstance(ws, list) and ws[0] == 0.0 and ws[1] == 1.0 / 3.0 and ws[2] == 1.0 / 3.0


def test_table_is_sound():
    ids = [c.id for c in F.CASES]
    assert len(set(ids)) == len(ids) and 24 <= len(ids) <= 72
    for c in F.CASES:
        assert c.family in F.FAMILIES and c.mode in (F.NORMAL, F.TRANS) and 1 <= c.k <= 16
        assert "SPL_LU_IRSTEP" not in c.env and all(isinstance(v, str) for v in c.env.values())
        assert "SPL_LU_STATIC_PIVOT" not in c.env or c.env["SPL_LU_STATIC_PIVOT"] == "0"  # path 5 is left out
        assert F.matrix(*c.matrix).shape[0] <= 14000
    for mode in (F.NORMAL, F.TRANS):  # every family both ways
        assert {c.family for c in F.CASES if c.mode == mode} == set(F.FAMILIES)
    assert {c.k for c in F.CASES} >= {1, 3, 8, 9}
    ns = {F.matrix(*c.matrix).shape[0] for c in F.CASES}
    assert 1 in ns and any(n % 32 for n in ns if n > 1)
    long_rows = [c for c in F.CASES if F.matrix(*c.matrix).nnz > 12 * F.matrix(*c.matrix).shape[0]]
    assert long_rows and any(c.report == "exact" for c in long_rows)  # the residual kernel with eight lanes per row


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_reference_raw_walk_is_at_rounding_level(case):
    """scipy's SuperLU without refinement on every input of the table: the yardstick has to be good before anything is
    held against it (measured: 4.5e-16 .. 2.8e-15 on the real meshes, up to 8.2e-15 on the complex ones)"""
    w = F.reference_omega(case)
    print("%s: omega_ref %s" % (case.id, " ".join("%.2e" % v for v in w)))
    assert len(w) == case.k and max(w) <= F.REF_LIMIT


def test_profile_holds_every_case_and_a_bound_per_family():
    """profiles/first_walk_omega.json (tools/first_walk_report.py): R is the smallest power of two at least twice the
    worst measured ratio of its family, and no family is above the limit"""
    with open(F.PROFILE) as f:
        prof = json.load(f)
    assert {r["id"] for r in prof["cases"]} == {c.id for c in F.CASES}
    for fam in F.FAMILIES:
        worst = max(r["ratio"] for r in prof["cases"] if r["family"] == fam)
        assert prof["worst_ratio"][fam] == worst
        R = prof["R"][fam]
        assert R == 2.0 ** round(math.log2(R)) and 2.0 * worst <= R < 4.0 * worst or (worst == 0.0 and R == 1.0)
        assert R <= F.R_LIMIT
