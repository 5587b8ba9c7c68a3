"""Inputs, switches and the yardstick of tests/test_gpu_first_walk.py, shared with tests/test_first_walk_cpu.py and
tools/first_walk_report.py.

Every case is a matrix, the environment that selects a code path of the LU (factor side or solve side), a system
(UmfpackNormal / UmfpackTrans) and a number of right-hand sides.  The GPU test solves it with SPL_LU_IRSTEP=0: what is
delivered is then the raw walk over the factors, and its componentwise backward error — evaluated exactly on the host,
helpers.exact_backward_error — is held against that of an independent LU of the same matrix without refinement
(scipy's SuperLU: another ordering, another pivoting), times a constant R per family.  R comes from
profiles/first_walk_omega.json (tools/first_walk_report.py measures the ratios and writes the file).

Everything here runs on the CPU; `python tests/first_walk_cases.py` prints the reference's figure of every case."""
import collections
import functools
import json
import os

import numpy as np
import scipy.sparse as sp

from helpers import exact_backward_error

NORMAL, TRANS = 0, 1  # umfpack.UmfpackNormal, umfpack.UmfpackTrans
U53 = 2.0 ** -53
R_LIMIT = 64.0        # no family may need more than this without a written cause
REF_LIMIT = 1e-14     # the reference's own raw walk has to stay below this on every input, or the input is replaced

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "first_walk_omega.json")


# ---- matrices (scipy CSC, sorted indices) ------------------------------------------------------------------------------
def _lap1(m):
    return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], (-1, 0, 1))


def _poisson(dim, m):
    """5-point (dim 2) / 7-point (dim 3) Laplacian on an m^dim grid: diagonal 2 dim, off-diagonals -1"""
    I, T = sp.identity(m), _lap1(m)
    if dim == 2:
        return sp.kron(I, T) + sp.kron(T, I)
    return sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)


def _dominant_by_columns(n, rows, cols, vals):
    """the entries given (duplicates summed, diagonal ones dropped) plus a diagonal of 1 + the column's absolute sum"""
    off = rows != cols
    A0 = sp.csc_matrix((vals[off], (rows[off], cols[off])), shape=(n, n))
    A0.sum_duplicates()
    return A0 + sp.diags(np.asarray(abs(A0).sum(axis=0)).ravel() + 1.0)


@functools.lru_cache(maxsize=None)
def matrix(name, m):
    rng = np.random.default_rng(1000 + m)
    if name in ("poisson3d", "poisson2d"):
        S = _poisson(int(name[7]), m)
    elif name in ("unsym3d", "unsym2d"):
        # column-dominant, unsymmetric values on the mesh pattern: off-diagonals x U(0.8, 1.2), diagonal 7
        C = sp.coo_matrix(_poisson(int(name[5]), m))
        v = C.data * rng.uniform(0.8, 1.2, C.nnz)
        v[C.row == C.col] = 7.0
        S = sp.csc_matrix((v, (C.row, C.col)), shape=C.shape)
    elif name == "complex3d":
        n = m ** 3
        S = (3.0 + 0.5j) * sp.identity(n) - _poisson(3, m)
    elif name == "blocks2x2":
        # 2 x 2 diagonal blocks [[1e-14, 3], [3, 1e-14]] plus a weak coupling m apart: useless pivots in the given
        # order, taken by threshold pivoting inside the diagonal blocks of the fronts
        n = m * m
        off = np.zeros(n - 1)
        off[0::2] = 3.0
        S = sp.diags([off, np.full(n, 1e-14), off, rng.uniform(-0.1, 0.1, n - m)], (-1, 0, 1, m))
    elif name == "random":
        # a random unsymmetric pattern with a dense-ish row and column, dominant by columns; 3.3 m entries
        rows = np.concatenate([rng.integers(0, m, 3 * m), np.full(m // 3, 7), rng.integers(0, m, m // 3)])
        cols = np.concatenate([rng.integers(0, m, 3 * m), rng.integers(0, m, m // 3), np.full(m // 3, 11)])
        S = _dominant_by_columns(m, rows, cols, rng.normal(size=len(rows)))
    elif name == "longrows":
        # 20 random entries per row: nnz > 12 n, the residual kernel with eight lanes per row
        rows, cols = np.repeat(np.arange(m), 20), rng.integers(0, m, 20 * m)
        S = _dominant_by_columns(m, rows, cols, rng.normal(size=len(rows)))
    elif name == "one":
        S = sp.csc_matrix(np.array([[3.0]]))
    else:
        raise KeyError(name)
    S = sp.csc_matrix(S)
    S.sort_indices()
    return S


def operator(case):
    """the matrix of the system the case solves: A, or A^T (A^H for complex A)"""
    S = matrix(*case.matrix)
    return S if case.mode == NORMAL else sp.csc_matrix(S.conj().T)


@functools.lru_cache(maxsize=None)
def _rhs(mat, mode, k):
    S = matrix(*mat)
    op = S if mode == NORMAL else sp.csc_matrix(S.conj().T)
    n = S.shape[0]
    rng = np.random.default_rng(7 * n + 100 * mode + k)
    cplx = np.iscomplexobj(S.data)
    out = []
    for _ in range(k):
        xs = rng.uniform(0.5, 1.5, n) + (1j * rng.uniform(-1.0, 1.0, n) if cplx else 0.0)
        b = np.asarray(op @ xs).ravel()
        b.setflags(write=False)
        out.append(b)
    return tuple(out)


def rhs(case):
    """the k right-hand sides of a case (manufactured: op @ xs, xs uniform in [0.5, 1.5), complex ones + i [-1, 1))"""
    return _rhs(case.matrix, case.mode, case.k)


@functools.lru_cache(maxsize=None)
def _reference(mat, mode, k):
    import scipy.sparse.linalg as spla
    S = matrix(*mat)
    op = sp.csc_matrix(S if mode == NORMAL else S.conj().T)
    lu = spla.splu(op)  # no refinement; COLAMD and threshold partial pivoting, independent of the product's choices
    bs = _rhs(mat, mode, k)
    xs = [lu.solve(np.array(b)) for b in bs]
    return tuple(exact_backward_error(op, xs, bs))


def reference_omega(case):
    """the exact backward error of the reference's raw solution, column by column"""
    return _reference(case.matrix, case.mode, case.k)


# ---- switches ------------------------------------------------------------------------------------------------------------
MF = {"SPL_LU_METHOD": "mf"}
SMALL = dict(MF, SPL_MF_SMALL="64", SPL_MF_MIDMAX="512", SPL_MF_BIGSOLVE="64")  # every class of front in a 24^3 tree
STEPS = dict(SMALL, SPL_MF_CHAIN="0")    # the substitution steps of the large fronts
CHAIN = dict(SMALL, SPL_MF_CHAIN="256")  # chains of 256 pivots: the 576 of the root are three blocks, the last one short
BAND = {"SPL_LU_METHOD": "band"}

Case = collections.namedtuple("Case", "id family matrix env mode k path path_after walks chain complex_fronts "
                                      "block_pivoting report")
# family: which R of the profile bounds it.  path / path_after: fact.path before and after the solve.  chain: the
# chain_span the report has to show (0: none, chain_bytes == 0).  report: "exact" — the reported backward error is
# held against the helper's to 1e-10; "rows" — the plain residual form, within (longest row + 2) roundings; None —
# the object solves a congruence of the embedding (SPL_ZI_SYMMETRIC=1), its figure belongs to other rows.


def _c(id, family, matrix, env, mode=NORMAL, k=1, path=3, path_after=None, walks=1, chain=0, complex_fronts=0,
       block_pivoting=0, report="exact"):
    return Case(id, family, matrix, dict(env), mode, k, path, path if path_after is None else path_after, walks, chain,
                complex_fronts, block_pivoting, report)


P24, U24, Z24 = ("poisson3d", 24), ("unsym3d", 24), ("complex3d", 24)

CASES = [
    # band, no interchanges: both forms of the diagonal blocks, both systems, a batch padded to the solve group
    _c("band-blocked-N", "band", ("unsym3d", 14), BAND, NORMAL, path=1),
    _c("band-blocked-T-k3", "band", ("unsym3d", 14), BAND, TRANS, k=3, path=1),
    _c("band-plaindiag-N", "band", ("unsym2d", 45), dict(BAND, SPL_LU_DIAG="plain"), NORMAL, path=1),
    _c("band-plaindiag-T", "band", ("unsym2d", 45), dict(BAND, SPL_LU_DIAG="plain"), TRANS, path=1),
    _c("band-poisson2d-110", "band", ("poisson2d", 110), BAND, NORMAL, path=1),
    # band, partial pivoting
    _c("band-pivot-N-k9", "band", ("unsym3d", 14), {"SPL_LU_FORCE_PIVOT": "1"}, NORMAL, k=9, path=0),
    _c("band-pivot-T", "band", ("unsym3d", 14), {"SPL_LU_FORCE_PIVOT": "1"}, TRANS, path=0),
    _c("band-pivot-blocks2x2", "band", ("blocks2x2", 40), {"SPL_LU_FORCE_PIVOT": "1"}, NORMAL, path=0),
    # tree, default limits (chains of 512 by default: the 576 pivots of the root are two blocks)
    _c("tree-default-ldlt-N", "chain", P24, MF, NORMAL, chain=512),
    _c("tree-default-lu-T", "chain", U24, MF, TRANS, chain=512),
    _c("tree-default-lu-N-n3375", "chain", ("unsym3d", 15), MF, NORMAL, chain=512),
    # tree, small limits, substitution steps: pipeline and split forward pass on and off, both systems
    _c("steps-pipe1-split1-N", "tree", U24, dict(STEPS, SPL_MF_PIPE="1", SPL_MF_SPLIT_FWD="1"), NORMAL),
    _c("steps-pipe1-split1-T", "tree", U24, dict(STEPS, SPL_MF_PIPE="1", SPL_MF_SPLIT_FWD="1"), TRANS),
    _c("steps-pipe0-split1-N", "tree", U24, dict(STEPS, SPL_MF_PIPE="0", SPL_MF_SPLIT_FWD="1"), NORMAL),
    _c("steps-pipe1-split0-T", "tree", U24, dict(STEPS, SPL_MF_PIPE="1", SPL_MF_SPLIT_FWD="0"), TRANS),
    _c("steps-pipe0-split0-N", "tree", U24, dict(STEPS, SPL_MF_PIPE="0", SPL_MF_SPLIT_FWD="0"), NORMAL),
    _c("steps-pipe0-split1-T", "tree", U24, dict(STEPS, SPL_MF_PIPE="0", SPL_MF_SPLIT_FWD="1"), TRANS),
    _c("steps-pipe1-split0-N", "tree", U24, dict(STEPS, SPL_MF_PIPE="1", SPL_MF_SPLIT_FWD="0"), NORMAL),
    _c("steps-pipe0-split0-T", "tree", U24, dict(STEPS, SPL_MF_PIPE="0", SPL_MF_SPLIT_FWD="0"), TRANS),
    _c("steps-ldlt-N", "tree", P24, STEPS, NORMAL),
    _c("steps-ldlt-T-k3", "tree", P24, STEPS, TRANS, k=3),
    _c("steps-lu-of-symmetric-N", "tree", P24, dict(STEPS, SPL_LU_SYMMETRIC="0"), NORMAL),
    _c("steps-lu-N-k9", "tree", U24, STEPS, NORMAL, k=9),
    _c("steps-lu-T-k9", "tree", U24, STEPS, TRANS, k=9),
    _c("steps-poisson2d-110", "tree", ("poisson2d", 110), STEPS, NORMAL),
    # chains of 256, one right-hand side, and with 8 and 9 columns (two groups, the second padded)
    _c("chain256-ldlt-N", "chain", P24, CHAIN, NORMAL, chain=256),
    _c("chain256-lu-N", "chain", U24, CHAIN, NORMAL, chain=256),
    _c("chain256-lu-T", "chain", U24, CHAIN, TRANS, chain=256),
    _c("chain256-lu-of-symmetric-T", "chain", P24, dict(CHAIN, SPL_LU_SYMMETRIC="0"), TRANS, chain=256),
    _c("chain256-multi-N-k8", "chain", U24, CHAIN, NORMAL, k=8, chain=256),
    _c("chain256-multi-T-k9", "chain", U24, CHAIN, TRANS, k=9, chain=256),
    _c("chain256-multi-ldlt-N-k9", "chain", P24, CHAIN, NORMAL, k=9, chain=256),
    _c("chain256-multi-off-N-k9", "chain", U24, dict(CHAIN, SPL_MF_CHAIN_MULTI="0"), NORMAL, k=9, chain=256),
    # the factor side: lookahead, paired lockstep steps, assembly beside the factorisation, the tree cut into subtrees
    _c("factor-lookahead1-N", "tree", U24, dict(STEPS, SPL_MF_MIDMAX="256", SPL_LU_LOOKAHEAD="1"), NORMAL),
    _c("factor-lookahead0-T", "tree", U24, dict(STEPS, SPL_MF_MIDMAX="256", SPL_LU_LOOKAHEAD="0"), TRANS),
    _c("factor-lookahead1-ldlt", "tree", P24, dict(STEPS, SPL_MF_MIDMAX="256", SPL_LU_LOOKAHEAD="1"), NORMAL),
    _c("factor-midpair1-N", "tree", P24, dict(STEPS, SPL_MF_MIDMAX="4096", SPL_MF_MIDPAIR="1"), NORMAL),
    _c("factor-midpair0-N", "tree", P24, dict(STEPS, SPL_MF_MIDMAX="4096", SPL_MF_MIDPAIR="0"), NORMAL),
    _c("factor-midpair1-lu-T", "tree", U24, dict(STEPS, SPL_MF_MIDMAX="4096", SPL_MF_MIDPAIR="1"), TRANS),
    _c("factor-overlap0-N", "tree", U24, dict(STEPS, SPL_MF_OVERLAP="0"), NORMAL),
    _c("factor-cut2-T", "tree", U24, dict(STEPS, SPL_MF_CUT="2"), TRANS),
    # complex: native fronts (substitution steps, chains, 8 complex columns = 16 real ones), and the real embeddings
    # (the general one with swapped pairs is not dominant and pivots inside its blocks; the symmetric one is L D L^T)
    _c("complex-native-steps-N", "complex", Z24, dict(STEPS, SPL_ZI_NATIVE="1"), NORMAL, path=4, complex_fronts=1),
    _c("complex-native-steps-T-k3", "complex", Z24, dict(STEPS, SPL_ZI_NATIVE="1"), TRANS, k=3, path=4,
       complex_fronts=1),
    _c("complex-native-chain256-N", "complex", Z24, dict(CHAIN, SPL_ZI_NATIVE="1"), NORMAL, path=4, chain=256,
       complex_fronts=1),
    # (22^3: one of the nine columns of the transposed system puts the reference at 1.5e-14 on 24^3; the root of 22^3
    # has 484 pivots, two blocks with a short last one)
    _c("complex-native-chain256-T-k9", "complex", ("complex3d", 22), dict(CHAIN, SPL_ZI_NATIVE="1"), TRANS, k=9, path=4,
       chain=256, complex_fronts=1),
    _c("complex-native-chain256-N-k8", "complex", Z24, dict(CHAIN, SPL_ZI_NATIVE="1"), NORMAL, k=8, path=4, chain=256,
       complex_fronts=1),
    _c("complex-embedding-general-N", "complex", ("complex3d", 16), dict(STEPS, SPL_ZI_NATIVE="0", SPL_ZI_SYMMETRIC="0"),
       NORMAL, path=4, block_pivoting=1),
    _c("complex-embedding-general-T", "complex", ("complex3d", 16), dict(STEPS, SPL_ZI_NATIVE="0", SPL_ZI_SYMMETRIC="0"),
       TRANS, path=4, block_pivoting=1),
    _c("complex-embedding-symmetric-N", "complex", ("complex3d", 16), dict(STEPS, SPL_ZI_NATIVE="0", SPL_ZI_SYMMETRIC="1"),
       NORMAL, path=4, report=None),
    _c("complex-embedding-symmetric-T", "complex", ("complex3d", 16), dict(STEPS, SPL_ZI_NATIVE="0", SPL_ZI_SYMMETRIC="1"),
       TRANS, path=4, report=None),
    # threshold pivoting inside the diagonal blocks (a speculation that holds), random patterns, long rows, edges
    _c("blockpivot-N", "chain", ("blocks2x2", 40), MF, NORMAL, path=4, chain=512, block_pivoting=1),
    _c("blockpivot-T-k3", "chain", ("blocks2x2", 40), MF, TRANS, k=3, path=4, chain=512, block_pivoting=1),
    # (the reference itself loses the transposed random systems with their dense row: 2.9e-14 at n = 700, 2.1e-13 at
    # n = 1 500 — the table takes the transposed one at n = 333, where it stays at 3.0e-15)
    _c("random-700-N", "chain", ("random", 700), MF, NORMAL, chain=512),
    _c("random-1500-N", "chain", ("random", 1500), MF, NORMAL, chain=512),
    _c("random-333-T", "chain", ("random", 333), MF, TRANS, chain=512),
    _c("longrows-500-N-k3", "chain", ("longrows", 500), MF, NORMAL, k=3, chain=512),
    _c("longrows-500-T-band", "band", ("longrows", 500), BAND, TRANS, path=1),
    _c("one-by-one", "band", ("one", 1), {}, NORMAL, path=1),
    # the plain residual form (three kernels): its figure carries a row length of roundings of its own
    _c("plainresidual-steps-N-k3", "tree", U24, dict(STEPS, SPL_LU_RESIDUAL="plain"), NORMAL, k=3, report="rows"),
    _c("plainresidual-longrows-T", "chain", ("longrows", 500), dict(MF, SPL_LU_RESIDUAL="plain"), TRANS, chain=512,
       report="rows"),
    # a speculation whose raw walk is useless (block pivoting off, no static pivoting): the ladder replaces the
    # factors by the pivoted band inside the same call, and what is delivered is that band's raw walk — two walks
    _c("replaced-speculation", "band", ("blocks2x2", 40), dict(MF, SPL_LU_BLOCK_PIVOT="0", SPL_LU_STATIC_PIVOT="0"),
       NORMAL, path=4, path_after=0, walks=2),
    _c("replaced-speculation-plainresidual", "band", ("blocks2x2", 40),
       dict(MF, SPL_LU_BLOCK_PIVOT="0", SPL_LU_STATIC_PIVOT="0", SPL_LU_RESIDUAL="plain"), NORMAL, path=4, path_after=0,
       walks=2, report="rows"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
FAMILIES = ("band", "tree", "chain", "complex")

# every switch a case may set: the GPU test clears the others, so that a case runs under its own environment only
SWITCHES = sorted(set(k for c in CASES for k in c.env) | {"SPL_LU_IRSTEP", "SPL_LU_GMRES", "SPL_MF_CHAIN_RB"})


def product_matrix(pkg, case):
    S = matrix(*case.matrix)
    n = S.shape[0]
    return pkg.Matrix(n, n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data)


def solve(pkg, fact, A, case):
    """the case's k systems through the entry point for one (k = 1) or many right-hand sides; the list of solutions"""
    U = pkg.umfpack
    bs = rhs(case)
    if case.k == 1:
        return [U.linearSolve_(fact, case.mode, A, bs[0])]
    return U.linearSolveMany_(fact, case.mode, A, list(bs))


def run_case(pkg, case):
    """Factor and solve once, under the environment the caller has put in place (the case's own and SPL_LU_IRSTEP).
    Returns the factors, the matrix and what was seen: path before and after, stats, the solve report, and the exact
    backward error of every delivered column."""
    U = pkg.umfpack
    A = product_matrix(pkg, case)
    fact = U.factor(A, U.analyze(A))
    seen = {"path": fact.path, "stats": fact.stats}
    xs = solve(pkg, fact, A, case)
    seen["report"] = fact.solve_report
    seen["path_after"] = fact.path
    seen["omega"] = exact_backward_error(operator(case), xs, list(rhs(case)))
    return fact, A, seen


def ratio(case, omega):
    """the worst column's exact backward error over the reference's for the same column (floored at 2^-53)"""
    return max(w / max(r, U53) for w, r in zip(omega, reference_omega(case)))


def longest_row(case):
    op = sp.csr_matrix(operator(case))
    if np.iscomplexobj(op.data):
        return 2 * int(np.max(np.diff(op.indptr)))
    return int(np.max(np.diff(op.indptr)))


def load_profile():
    with open(PROFILE) as f:
        return json.load(f)


def bound_factor(case, profile=None):
    """R of the case's family (the profile's, measured on the device; never above R_LIMIT without a recorded cause)"""
    profile = profile or load_profile()
    return float(profile["R"][case.family])


if __name__ == "__main__":  # the reference's own figure of every case, without a GPU
    import time
    for c in CASES:
        t0 = time.time()
        w = reference_omega(c)
        print("%-40s n %6d  k %d  omega_ref %.2e  (%.1f s)" % (c.id, matrix(*c.matrix).shape[0], c.k, max(w),
                                                               time.time() - t0))
