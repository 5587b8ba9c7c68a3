"""The raw walk over the LU factors (SPL_LU_IRSTEP=0) on every path of tests/first_walk_cases.py: what one pass through
the factorisation and substitution kernels delivers, before iterative refinement can repair it.  Two refinement steps
contract an error of 1e-6 in the factors to rounding level, so the assertions on refined solutions elsewhere in the
suite cannot see it; the exact backward error of the unrefined solution can.

For every case: the report says one walk and no refinement step (two walks where the ladder replaces the factors),
the path is the expected one before and after, every column's exact componentwise backward error is at most
R x max(omega_ref, 2^-53) — omega_ref the same figure of scipy's SuperLU without refinement for the same column, R the
family's constant of profiles/first_walk_omega.json (measured, at most 64) —, and the backward error the product
reports is the exact one of the worst column.  Then the same object solves again with the default refinement."""
import numpy as np
import pytest

import first_walk_cases as F
from helpers import exact_backward_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def profile():
    return F.load_profile()


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_first_walk(gpu, pkg, case, profile, monkeypatch):
    for name in F.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setenv("SPL_LU_IRSTEP", "0")
    fact, A, seen = F.run_case(pkg, case)
    rep, st = seen["report"], seen["stats"]
    ref = F.reference_omega(case)
    R = F.bound_factor(case, profile)
    assert R <= F.R_LIMIT
    worst = max(seen["omega"])
    print("%s: path %d -> %d, walks %d, chain %d (%.0f bytes); omega %s; reference %s; worst ratio %.2f of R = %g; "
          "reported %.17g, exact %.17g" % (case.id, seen["path"], seen["path_after"], rep["walks"], rep["chain_span"],
                                           rep["chain_bytes"], " ".join("%.2e" % w for w in seen["omega"]),
                                           " ".join("%.2e" % w for w in ref), F.ratio(case, seen["omega"]), R,
                                           rep["backward_error"], worst))
    # the case ran the code it is in the table for
    assert (seen["path"], seen["path_after"]) == (case.path, case.path_after)
    assert rep["walks"] == case.walks and rep["ir_attempted"] == 0 and rep["ir_taken"] == 0
    assert st["complex_fronts"] == case.complex_fronts and st["block_pivoting"] == case.block_pivoting
    assert rep["chain_span"] == case.chain and (rep["chain_bytes"] > 0) == (case.chain > 0)
    assert (case.family != "chain" or rep["chain_bytes"] > 0) and (case.family != "tree" or rep["chain_bytes"] == 0)
    # the raw walk is as good as an independent LU's, column by column
    for c, (w, r) in enumerate(zip(seen["omega"], ref)):
        assert w <= R * max(r, F.U53), (case.id, c, w, r)
    # the figure the product reports (and accepts speculative factors by) is that of what it delivered
    if case.report == "exact":
        assert abs(rep["backward_error"] - worst) <= 1e-10 * worst
    elif case.report == "rows":
        # the plain form subtracts a rounded product: at most (row length + 1) roundings of the denominator's size
        assert abs(rep["backward_error"] - worst) <= (F.longest_row(case) + 2) * F.U53 * (1.0 + 1e-10)
    # the same object with the default refinement: what the other tests of the suite ask of it
    monkeypatch.delenv("SPL_LU_IRSTEP")
    xs = F.solve(pkg, fact, A, case)
    rep2 = fact.solve_report
    assert fact.path == case.path_after
    assert rep2["walks"] == 1 + rep2["ir_attempted"] and rep2["ir_attempted"] <= (10 if fact.path in (2, 4) else 2)
    # (below eps on the dominant meshes and the native complex fronts, as the tests of those paths have it; elsewhere
    # the level speculative factors are accepted at)
    mesh = case.matrix[0] in ("poisson3d", "poisson2d", "unsym3d", "unsym2d")
    assert rep2["backward_error"] <= (2.3e-16 if (mesh and case.path_after == 3) or case.complex_fronts else 1e-13)
    for w, r in zip(exact_backward_error(F.operator(case), xs, list(F.rhs(case))), ref):
        assert w <= R * max(r, F.U53)


def test_irstep_counts_the_steps_it_allows(gpu, pkg, monkeypatch):
    """SPL_LU_IRSTEP=k is the number of refinement steps a call may take, read at every call; anything that is not an
    integer in 0 .. 10 leaves the defaults"""
    case = F.BY_ID["steps-lu-N-k9"]
    for name in F.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    U = pkg.umfpack
    A = F.product_matrix(pkg, case)
    fact = U.factor(A, U.analyze(A))
    b = F.rhs(case)[0]
    x_default = U.linearSolve_(fact, case.mode, A, b)
    default = fact.solve_report
    assert 1 <= default["ir_attempted"] <= 2
    for value, steps in (("0", 0), ("1", 1), ("2", default["ir_attempted"]), ("11", default["ir_attempted"]),
                         ("-1", default["ir_attempted"]), ("x", default["ir_attempted"]), ("", default["ir_attempted"])):
        monkeypatch.setenv("SPL_LU_IRSTEP", value)
        x = U.linearSolve_(fact, case.mode, A, b)
        rep = fact.solve_report
        assert (rep["ir_attempted"], rep["walks"]) == (steps, 1 + steps), value
        if steps == default["ir_attempted"]:
            assert np.array_equal(x, x_default)
        assert abs(rep["backward_error"] - exact_backward_error(F.operator(case), x, b)) <= 1e-10 * rep["backward_error"]
