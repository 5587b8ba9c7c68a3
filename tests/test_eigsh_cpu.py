"""The restatement of tests/eigsh_cases.py checked on its own, without a GPU: on every committed case it converges inside
its max_restarts, every value it returns is an eigenvalue by numpy.linalg.eigvalsh within the Hermitian residual bound,
the values are the wanted ones, and the residual estimate of the close is honest."""
import numpy as np
import pytest

import eigsh_cases as EK
import krylov_cases as K

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def spectrum():
    cache = {}

    def of(name):
        if name not in cache:
            cache[name] = np.linalg.eigvalsh(EK.matrix(name).toarray())
        return cache[name]
    return of


def floor_of(S):
    """64 n 2^-53 |A|_inf: the rounding of the residual and of numpy"""
    return 64.0 * S.shape[0] * EPS * EK.norm_inf(S)


def check_values(out, S, exact, wanted):
    """every value within residual / |x| + floor of an eigenvalue, and the values are `wanted` within the same bound"""
    floor = floor_of(S)
    assert out.pairs == len(wanted)
    for i in range(out.pairs):
        bound = out.residuals[i] / np.linalg.norm(out.vectors[:, i]) + floor
        print("value %.17g  nearest %.3e  wanted %.3e  bound %.3e" % (out.values[i], np.min(np.abs(exact - out.values[i])),
                                                                 abs(out.values[i] - wanted[i]), bound))
        assert np.min(np.abs(exact - out.values[i])) <= bound
        assert abs(out.values[i] - wanted[i]) <= bound


@pytest.mark.parametrize("case", EK.DIRECT, ids=lambda c: "-".join(str(v) for v in c))
def test_direct_cases_converge_to_numpy_s_extreme_values(spectrum, case):
    name, which, nev, ncv, tol, max_restarts = case
    S = EK.matrix(name)
    exact = spectrum(name)
    out = EK.reference(*case)
    assert out.reason == 0 and 1 <= out.cycles <= max_restarts
    assert len(out.history) == out.cycles + 1 and 1 <= out.sweeps <= EK.MAX_SWEEPS
    if which == "LA":
        wanted = exact[::-1][:nev]
    elif which == "SA":
        wanted = exact[:nev]
    else:
        wanted = exact[np.argsort(-np.abs(exact), kind="stable")][:nev]
    gaps = np.abs(np.diff(np.sort(exact)))
    assert gaps.min() > 1e3 * floor_of(S), "the committed matrices have simple eigenvalues"
    check_values(out, S, exact, wanted)
    # the estimate of the close against the true residual: the check a drop test on |t a| fails
    floor = floor_of(S)
    for i in range(out.pairs):
        print("residual %.3e  estimate %.3e" % (out.residuals[i], out.estimates[i]))
        assert out.residuals[i] <= 2.0 * max(out.estimates[i], floor)
        assert out.estimates[i] <= max(tol * abs(out.values[i]), 0.0)
    assert out.history[-1] == out.estimates.max()


@pytest.mark.parametrize("sigma,M,nev,ncv", [c for c in EK.INVERSE if c[1] != "amg"])
def test_inverse_cases_find_the_values_nearest_sigma(spectrum, sigma, M, nev, ncv):
    S = EK.matrix("grid")
    exact = spectrum("grid")
    out = EK.inverse_reference(sigma, M, nev, ncv)
    assert out.reason == 0 and out.inner > 0 and out.ops >= ncv
    wanted = exact[np.argsort(np.abs(exact - sigma), kind="stable")][:nev]
    check_values(out, S, exact, wanted)


def test_inner_solve_that_fails_is_reason_4():
    out = EK.inverse_reference(0.0, None, 3, 12, max_iter=1)
    assert out.reason == 4 and out.pairs == 0 and out.ops == 0 and out.inner == 1 and out.cycles == 0


def test_outcomes_of_the_header():
    import scipy.sparse as sp
    two = sp.csr_matrix(2.0 * sp.identity(16))
    ones = np.ones(16)  # v_0 = 1/4 in every entry: <v_0,v_0> is 1 exactly, and w - 2 v_0 is 0 exactly
    out = EK.eigsh(two, ones, 1, "LA", 4)
    assert out.result == [0, 1, 1, 1, 0, 0] and out.values[0] == 2.0
    out = EK.eigsh(two, ones, 2, "LA", 4)
    assert out.reason == 2 and out.pairs == 1 and out.ops == 1
    D = sp.csr_matrix(sp.diags([np.arange(1.0, 7.0)], [0]))
    e1 = np.zeros(6)
    e1[0] = 1.0
    out = EK.eigsh(D, e1, 1, "LA", 4)
    assert out.reason == 0 and out.ops == 1 and out.values[0] == 1.0 and out.residuals[0] == 0.0
    out = EK.eigsh(D, np.zeros(6), 1, "LA", 4)
    assert out.reason == 2 and out.pairs == 0 and out.history[0] == 0.0
    bad = sp.csr_matrix(sp.diags([[1.0, np.inf, 3.0, 4.0, 5.0, 6.0]], [0]))
    out = EK.eigsh(bad, EK.start_vector(6), 1, "LA", 4)
    assert out.reason == 3 and out.pairs == 0
    out = EK.reference("ramp", "SA", 3, 12, 1e-10, 1)
    assert out.reason == 1 and out.cycles == 1 and out.pairs == 3


@pytest.mark.parametrize("cplx", [False, True])
def test_rotation_is_the_product(cplx):
    rng = np.random.default_rng(5)
    V = rng.standard_normal((37, 9)) + (1j * rng.standard_normal((37, 9)) if cplx else 0.0)
    Y = rng.standard_normal((9, 4))
    got = EK.rotate(V, Y)
    assert got.dtype == V.dtype and np.allclose(got, V @ Y, rtol=1e-13, atol=1e-13)
    assert K.bits_equal(EK.rotate(V[:, :1], Y[:1, :1]), EK.real_times(float(Y[0, 0]), V[:, 0]).reshape(-1, 1))


def test_jacobi_diagonalises_an_arrow_head_with_a_tail():
    rng = np.random.default_rng(11)
    m, k = 14, 5
    T = np.zeros((m, m))
    T[np.arange(k), np.arange(k)] = rng.standard_normal(k)
    T[:k, k] = T[k, :k] = 1e-3 * rng.standard_normal(k)
    for j in range(k, m):
        T[j, j] = rng.standard_normal()
        if j < m - 1:
            T[j, j + 1] = T[j + 1, j] = abs(rng.standard_normal())
    theta, Y, sweeps = EK.jacobi([list(map(float, row)) for row in T])
    Y = np.array(Y)
    assert 1 <= sweeps <= 10
    assert np.allclose(np.sort(theta), np.linalg.eigvalsh(T), rtol=0.0, atol=1e-14 * np.abs(T).sum())
    assert np.allclose(Y.T @ Y, np.eye(m), atol=1e-14) and np.allclose(Y @ np.diag(theta) @ Y.T, T, atol=1e-14)
    assert EK.jacobi([[3.0]]) == ([3.0], [[1.0]], 0)
