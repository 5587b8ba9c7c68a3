"""Host tables of the sparse triangular solve (csrc/tri_levels.hpp): the triangle of every row, the level numbers, the
per-level row lists, the launch plan and its launch count (info[3] of spl_trisolve_info), and the transposed image are
plain C++, so they are checked on the CPU with a small native driver (tests/native/tri_levels_check.cpp) that restates
every table from the pattern alone.  The expectations written out below are counted by hand from the patterns."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS")
SHRUNK = {"SPL_TRSV_SMALL_ROWS": "8", "SPL_TRSV_SEGMENT_LEVELS": "5"}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tri_levels") / "tri_levels_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "sparse-linear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "tri_levels_check.cpp"), "-o", exe], check=True)
    return exe


def check(checker, S, lower, knobs=None):
    S = sp.csr_matrix(S)
    S.sort_indices()
    text = "%d %d %d\n%s\n%s\n" % (S.shape[0], S.nnz, int(lower), " ".join(map(str, S.indptr)),
                                   " ".join(map(str, S.indices)))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs or {})
    r = subprocess.run([checker], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert out["bad"] == 0
    return out


def poisson2d(m):
    T = sp.diags([-np.ones(m - 1), 4 * np.ones(m), -np.ones(m - 1)], (-1, 0, 1))
    E = sp.diags([-np.ones(m - 1), -np.ones(m - 1)], (-1, 1))
    return sp.csr_matrix(sp.kron(sp.identity(m), T) + sp.kron(E, sp.identity(m)))


def bidiagonal(n, lower=True):
    return sp.csr_matrix(sp.diags([np.ones(n), np.ones(n - 1)], (0, -1 if lower else 1)))


def random_lower(n, seed):
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=0.01, random_state=rng, format="csr")
    return sp.csr_matrix(sp.tril(A, -1) + sp.identity(n))


@pytest.mark.parametrize("knobs", [None, SHRUNK], ids=["default", "shrunk"])
def test_empty_one_and_diagonal(checker, knobs):
    out = check(checker, sp.csr_matrix((0, 0)), True, knobs)
    assert (out["n"], out["levels"], out["launches"], out["stored"]) == (0, 0, 0, 0)
    for lower in (True, False):
        out = check(checker, sp.identity(1, format="csr"), lower, knobs)
        assert (out["levels"], out["launches"], out["stored"], out["longest"]) == (1, 1, 1, 1)
        out = check(checker, sp.csr_matrix((1, 1)), lower, knobs)  # n = 1 with no stored entry
        assert (out["levels"], out["launches"], out["stored"], out["longest"]) == (1, 1, 0, 0)
        out = check(checker, sp.identity(500, format="csr"), lower, knobs)  # one level of 500 rows: wide either way
        assert (out["levels"], out["launches"], out["wide"], out["narrow"]) == (1, 1, 1, 0)


@pytest.mark.parametrize("lower", [True, False])
def test_bidiagonal_chain(checker, lower):
    A = bidiagonal(3000, lower)
    out = check(checker, A, lower)
    # 3000 levels of one row: all narrow, ceil(3000 / 1024) = 3 segments
    assert (out["levels"], out["wide"], out["narrow"], out["launches"], out["widest"]) == (3000, 0, 3, 3, 1024)
    assert (out["stored"], out["longest"]) == (5999, 2)
    out = check(checker, A, lower, {"SPL_TRSV_SEGMENT_LEVELS": "1"})
    assert (out["levels"], out["narrow"], out["launches"], out["widest"]) == (3000, 3000, 3000, 1)
    out = check(checker, A, lower, {"SPL_TRSV_SMALL_ROWS": "1"})  # nothing is below one row: every level wide
    assert (out["wide"], out["narrow"], out["launches"]) == (3000, 0, 3000)
    # the other triangle of the same matrix is its diagonal
    out = check(checker, A, not lower)
    assert (out["levels"], out["stored"], out["launches"]) == (1, 3000, 1)


@pytest.mark.parametrize("knobs", [None, SHRUNK], ids=["default", "shrunk"])
def test_dense_triangle(checker, knobs):
    A = sp.csr_matrix(np.tril(np.ones((70, 70))))
    out = check(checker, A, True, knobs)
    assert (out["levels"], out["stored"], out["longest"], out["wide"]) == (70, 70 * 71 // 2, 70, 0)
    assert out["launches"] == (1 if knobs is None else 14)  # 70 levels of one row, 5 to a segment
    out = check(checker, sp.csr_matrix(A.T), False, knobs)
    assert (out["levels"], out["longest"]) == (70, 70)


@pytest.mark.parametrize("lower", [True, False])
def test_poisson2d_levels_grow_and_shrink(checker, lower):
    A = poisson2d(40)
    T = sp.tril(A) if lower else sp.triu(A)
    for operand in (T, A):  # the other side of the diagonal is not read
        out = check(checker, operand, lower)
        # level = i + j of the grid point: 79 anti-diagonals of 1 ... 40 ... 1 points
        assert (out["levels"], out["stored"], out["longest"]) == (79, 1600 + 2 * 40 * 39, 3)
        assert (out["wide"], out["narrow"], out["launches"]) == (0, 1, 1)
        # SMALL = 8: the 7 first and 7 last levels are narrow (two segments of 5 + 2 each side), 65 are wide
        out = check(checker, operand, lower, SHRUNK)
        assert (out["wide"], out["narrow"], out["launches"]) == (65, 4, 69)
        out = check(checker, operand, lower, {"SPL_TRSV_SMALL_ROWS": "41"})
        assert (out["wide"], out["narrow"]) == (0, 1)
        out = check(checker, operand, lower, {"SPL_TRSV_SMALL_ROWS": "40"})
        assert (out["wide"], out["narrow"], out["launches"]) == (1, 2, 3)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_lower_pattern(checker, seed):
    A = random_lower(2000, seed)
    for knobs in (None, SHRUNK, {"SPL_TRSV_SMALL_ROWS": "1"}, {"SPL_TRSV_SMALL_ROWS": "100000"}):
        out = check(checker, A, True, knobs)
        assert out["levels"] > 2 and out["stored"] == A.nnz
    # a pattern without a diagonal, and the upper triangle of the transpose
    out = check(checker, sp.tril(A, -1), True)
    assert out["stored"] == A.nnz - 2000
    check(checker, sp.csr_matrix(A.T), False, SHRUNK)


def test_knobs_are_clamped(checker):
    A = bidiagonal(10)

    def read(**knobs):
        out = check(checker, A, True, knobs)
        return out["small"], out["segment"]

    assert read() == (64, 1024)
    assert read(SPL_TRSV_SMALL_ROWS="0", SPL_TRSV_SEGMENT_LEVELS="0") == (1, 1)
    assert read(SPL_TRSV_SMALL_ROWS="-5", SPL_TRSV_SEGMENT_LEVELS="-1") == (1, 1)
    assert read(SPL_TRSV_SMALL_ROWS="99999999999", SPL_TRSV_SEGMENT_LEVELS="99999999999") == (2 ** 30, 65536)
    assert read(SPL_TRSV_SMALL_ROWS="", SPL_TRSV_SEGMENT_LEVELS="many") == (64, 1024)
    assert read(SPL_TRSV_SMALL_ROWS="17", SPL_TRSV_SEGMENT_LEVELS="3") == (17, 3)
