"""The restatement of tests/globpcg_cases.py (LOBPCG for A x = lambda B x) checked on its own, without a GPU: its values
against the dense pencil that numpy builds from the Cholesky factor of B, the B-orthonormality of its vectors, its
equality with the standard restatement when B is an identity, and both copies of a double eigenvalue.  Also the symbols
and the Python surface (which fail without the feature), and what the calls answer before the device is touched.

The bounds.  For a B-normalised x with r = A x - theta B x, some eigenvalue of the pencil lies within
|r|_2 / sqrt(lambda_min(B)) of theta (the Hermitian residual bound on L^-1 A L^-H with B = L L^H); lambda_min(B) is
taken from numpy.  The floor beside it is the error of the reference itself: eigvalsh of C = L^-1 A L^-H is good to a few
2^-53 |C|, |C|_2 <= |A|_1 / lambda_min(B), and forming C through the factor costs another kappa_2(B):
8 2^-53 kappa_2(B) |A|_1 / lambda_min(B).
B-orthonormality: max |X^H B X - I| is bounded by 16 kappa_2(B) times max |X^H X - I| of the standard restatement on the
same A, block and start; 16 is headroom for the other inner product.  Measured (python tests/globpcg_cases.py), as
|X^H B X - I| / standard |X^H X - I| / bound:  poisson12 b6 3.1e-16 / 4.4e-16 / 5.9e-14;  phased12 b6 3.6e-16 / 2.2e-16 /
3.0e-14;  poisson12 b4 largest 4.4e-16 / 2.2e-16 / 3.0e-14;  two 2.2e-16 / 1.1e-16 / 3.6e-15;  kappa_2(mass12) = 8.335."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import globpcg_cases as GK
import lobpcg_cases as LK

EPS = 2.0 ** -53
SYMBOLS = {"spl_lobpcg_set_mass": 2, "spl_vector_update_pair_dev": 12}
HANDLE = -3
LOBPCG_MAGIC = 0x53504C42  # "SPLB": the word an spl_lobpcg_* call looks for at the head of its object

CONVERGING = [c for c in GK.CASES if c[0] != "grid70"]


def spectrum_of(S):
    return np.linalg.eigvalsh(S.toarray())


def pencil_values(S, Bm):
    """the eigenvalues of S x = lambda Bm x, ascending: eigvalsh(L^-1 S L^-H) with Bm = L L^H"""
    L = np.linalg.cholesky(Bm.toarray())
    Li = np.linalg.inv(L)
    Cm = Li @ S.toarray() @ Li.conj().T
    return np.linalg.eigvalsh((Cm + Cm.conj().T) / 2.0)


def check_against_the_dense_pencil(out, S, Bm, which, nev):
    """the matching rule of test_lobpcg_cpu.check_against_numpy with the bound of the module docstring"""
    exact = pencil_values(S, Bm)
    mass_values = spectrum_of(Bm)
    low, kappa = mass_values[0], mass_values[-1] / mass_values[0]
    wanted = np.sort(exact[::-1][:nev] if which == LK.LARGEST else exact[:nev])
    got = np.sort(out.values)
    by_value = np.argsort(out.values, kind="stable")
    floor = 8.0 * EPS * kappa * LK.norm_one(S) / low
    for k in range(nev):
        i = by_value[k]
        x = out.vectors[:, i]
        b_norm = np.sqrt(abs(np.vdot(x, Bm @ x)))
        bound = out.residuals[i] / b_norm / np.sqrt(low) + floor
        print("theta %.17g  wanted %.17g  |difference| %.3e  bound %.3e" % (got[k], wanted[k], abs(got[k] - wanted[k]), bound))
        assert abs(got[k] - wanted[k]) <= bound
    # the copies are independent: a B-orthonormal X has singular values of at least 1 / sqrt(lambda_max(B))
    smallest = np.linalg.svd(out.vectors, compute_uv=False).min()
    assert smallest >= 0.99 / np.sqrt(mass_values[-1])


@pytest.mark.parametrize("case", CONVERGING, ids=lambda c: "-".join(str(v) for v in c))
def test_cases_converge_to_the_dense_pencil_s_extreme_values(case):
    name, bname, block, nev, which, tol, max_iter = case
    out = GK.reference(*case)
    assert out.reason == 0 and out.pairs == nev and out.iterations <= max_iter
    assert len(out.history) == out.iterations + 1 and out.sweeps <= LK.MAX_SWEEPS
    assert out.history[-1] <= tol * np.abs(out.values).max()
    assert out.syncs == 2 + 2 * out.iterations + 2
    assert out.spmv_columns == block + 2 * block * out.iterations + nev
    assert out.mass_columns == block + block * out.iterations + nev
    check_against_the_dense_pencil(out, LK.matrix(name), GK.mass(bname), which, nev)


def test_grid70_stops_at_max_iter():
    out = GK.reference(*[c for c in GK.CASES if c[0] == "grid70"][0])
    assert out.reason == 1 and out.iterations == 3 and out.pairs == 2 and len(out.history) == 4


def test_preconditioned_case_converges():
    kind, block, nev, tol, max_iter = GK.PRECONDITIONED[0]
    assert kind == "jacobi"
    out = GK.reference("poisson8", "mass8_3d", block, nev, LK.SMALLEST, tol, max_iter, kind)
    assert out.reason == 0 and out.applications == block * out.iterations
    check_against_the_dense_pencil(out, LK.matrix("poisson8"), GK.mass("mass8_3d"), LK.SMALLEST, nev)


def kappa_of(bname):
    """kappa_2 of a committed mass matrix from the 1-D factor T = tridiag(1, 4, 1): a Kronecker power has the products of
    T's eigenvalues, and the phases are a unitary similarity"""
    if bname == "diag21":
        return 2.0
    m, power = {"mass12": (12, 2), "phased_mass12": (12, 2), "mass70": (70, 2), "mass8_3d": (8, 3)}[bname]
    t = np.linalg.eigvalsh(GK._tri141(m).toarray())
    return float((t[-1] / t[0]) ** power)


@pytest.mark.parametrize("case", GK.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_vectors_are_b_orthonormal(case):
    name, bname, block, nev, which, tol, max_iter = case
    gen = GK.reference(*case)
    std = LK.reference(name, block, nev, which, tol, max_iter)
    plain = float(np.abs(std.vectors.conj().T @ std.vectors - np.eye(std.pairs)).max())
    kappa = kappa_of(bname)
    assert kappa < 9.0 or bname == "mass8_3d"
    measured = GK.b_orthonormality(gen, GK.mass(bname))
    print("|X^H B X - I| %.3e  standard |X^H X - I| %.3e  kappa_2(B) %.3f  bound %.3e" % (measured, plain, kappa,
                                                                                          16.0 * kappa * plain))
    assert plain > 0.0 and measured <= 16.0 * kappa * plain


@pytest.mark.parametrize("case", [c for c in LK.CASES if c[0] in ("poisson12", "phased12", "five")],
                         ids=lambda c: "-".join(str(v) for v in c))
def test_an_identity_mass_gives_the_standard_restatement(case):
    name, block, nev, which, tol, max_iter = case
    S = LK.matrix(name)
    std = LK.reference(*case)
    gen = GK.lobpcg(S, GK.identity(S.shape[0], np.iscomplexobj(S.data)), LK.start_of(name, block), nev, which, tol, 0.0,
                    max_iter)
    assert gen.result == std.result
    assert np.array_equal(gen.values, std.values) and np.array_equal(gen.vectors, std.vectors)
    assert np.array_equal(gen.residuals, std.residuals) and np.array_equal(gen.history, std.history)
    assert gen.mass_columns == block + block * std.iterations + nev


def test_both_copies_of_the_double_eigenvalue_are_returned():
    S, Bm = LK.matrix("poisson12"), GK.mass("mass12")
    out = GK.reference("poisson12", "mass12", 6, 4, LK.SMALLEST, 1e-9, 200)
    exact = pencil_values(S, Bm)
    assert abs(exact[1] - exact[2]) < 1e-12 < exact[3] - exact[2]  # the pencil keeps the grid's transpose symmetry
    order = np.argsort(out.values, kind="stable")
    theta = out.values[order]
    assert abs(theta[1] - exact[1]) < 1e-9 and abs(theta[2] - exact[2]) < 1e-9
    x1, x2 = out.vectors[:, order[1]], out.vectors[:, order[2]]
    std = LK.reference("poisson12", 6, 4, LK.SMALLEST, 1e-9, 200)
    plain = float(np.abs(std.vectors.conj().T @ std.vectors - np.eye(std.pairs)).max())
    assert abs(np.vdot(x1, Bm @ x2)) <= 16.0 * kappa_of("mass12") * plain  # B-orthogonal, within the bound of the test above
    assert np.linalg.svd(np.stack([x1, x2], axis=1), compute_uv=False).min() > 0.1


def test_update_pair_of_the_restatement_is_two_updates_and_a_dot():
    rng = np.random.default_rng(5)
    V, BV = [rng.standard_normal(300) for _ in range(3)], [rng.standard_normal(300) for _ in range(3)]
    w, bw, coef = rng.standard_normal(300), rng.standard_normal(300), [0.5, -1.25, 3.0]
    w2, bw2, q = GK.update_pair(V, BV, coef, w, bw, GK.K.Real)
    assert np.array_equal(w2, ((w - 0.5 * V[0]) - -1.25 * V[1]) - 3.0 * V[2])
    assert np.array_equal(bw2, ((bw - 0.5 * BV[0]) - -1.25 * BV[1]) - 3.0 * BV[2])
    assert q == GK.K.Real.dot(w2, bw2)


def test_the_symbols_and_the_python_surface(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes and len(fn.argtypes) == nargs, name
    assert pkg.vector_update_pair_dev is pkg.sparse.vector_update_pair_dev
    assert callable(pkg.LOBPCGSolver.set_mass)
    for fn, last in ((pkg.LOBPCGSolver.__init__, ["self", "A", "block", "M", "B"]),
                     (pkg.DeviceMatrix.lobpcg, ["self", "X0", "nev", "largest", "M", "tol", "atol", "maxiter", "B"]),
                     (pkg.sparse.lobpcg, ["mat", "X0", "nev", "largest", "M", "tol", "atol", "maxiter", "B"])):
        params = inspect.signature(fn).parameters
        assert list(params) == last and params["B"].default is None  # the new keyword goes last
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sparse_linear_hip.h")).read()
    assert "A x = lambda B x, interior" not in header and "spl_lobpcg_set_mass(void *L, void *B)" in header


def test_what_is_no_handle_is_refused_before_the_device(pkg):
    L = pkg._ffi.lib()
    junk = C.create_string_buffer(256)
    assert L.spl_lobpcg_set_mass(junk, None) == HANDLE
    assert L.spl_lobpcg_set_mass(None, None) == HANDLE
    assert L.spl_lobpcg_set_mass(junk, junk) == HANDLE
    # behind an object's magic word the call looks at B next, and refuses what is no matrix handle before anything else
    # of the object is read
    fake = C.create_string_buffer(4096)
    C.memmove(fake, C.byref(C.c_uint32(LOBPCG_MAGIC)), 4)
    assert L.spl_lobpcg_set_mass(fake, junk) == HANDLE
    assert L.spl_lobpcg_set_mass(fake, fake) == HANDLE  # a solver object is no matrix


if __name__ == "__main__":
    for case in GK.CASES:
        test_the_vectors_are_b_orthonormal(case)
