"""The yardstick of tests/test_gpu_eigsh.py and tests/test_eigsh_cpu.py: a serial restatement of the section "thick-restart
Lanczos on handles" of include/sparse_linear_hip.h, built from the pieces of tests/krylov_cases.py (the fold, the
row-serial operator, the two arithmetics, CG for the inverse mode) and tests/gmres_cases.py (the scalars), plus the
cyclic Jacobi of the header in plain Python floats.  It never runs code of the library under test.

Every product, sum, quotient and root is one separately rounded IEEE operation.  A real number times an entry and an entry
over a real number are done part by part (numpy's float * complex is NOT that, so the parts are multiplied apart).
`python tests/eigsh_cases.py` prints what every committed case does, without a GPU."""
import functools
import math

import numpy as np
import scipy.sparse as sp

import gmres_cases as G
import krylov_cases as K
import trisolve_cases as TK

REASONS = ("converged", "max_restarts", "invariant_subspace", "non_finite", "inner_solve_failed")
WHICH = {"LA": 0, "SA": 1, "LM": 2}
MAX_SWEEPS = 60


# ---- the rotation --------------------------------------------------------------------------------------------------------
def real_times(y, v):
    """a real number times a vector, part by part"""
    with np.errstate(all="ignore"):
        if np.iscomplexobj(v):
            return K._cvec(y * v.real, y * v.imag)
        return y * v


def rotate(V, Y):
    """V Y: V an n x m array (float64 or complex128), Y a REAL m x k array.  Column i is x = Y[0][i] v_0;
    x = x + Y[l][i] v_l ascending, one product and one sum per term and part; all columns at once, term by term"""
    V, Y = np.asarray(V), np.asarray(Y, dtype=np.float64)
    m = V.shape[1]
    with np.errstate(all="ignore"):
        if np.iscomplexobj(V):
            re, im = np.ascontiguousarray(V.real), np.ascontiguousarray(V.imag)
            xr, xi = re[:, 0:1] * Y[0:1, :], im[:, 0:1] * Y[0:1, :]
            for l in range(1, m):
                xr = xr + re[:, l:l + 1] * Y[l:l + 1, :]
                xi = xi + im[:, l:l + 1] * Y[l:l + 1, :]
            out = np.empty(xr.shape, dtype=np.complex128)
            out.real, out.imag = xr, xi
            return out
        x = V[:, 0:1] * Y[0:1, :]
        for l in range(1, m):
            x = x + V[:, l:l + 1] * Y[l:l + 1, :]
        return x


# ---- cyclic Jacobi ---------------------------------------------------------------------------------------------------------
def jacobi(T):
    """(theta, Y, sweeps) of the real symmetric T (a list of lists of floats, changed in place), or None past MAX_SWEEPS"""
    m = len(T)
    Y = [[1.0 if r == c else 0.0 for c in range(m)] for r in range(m)]
    sweeps = 0
    while True:
        if not any(T[p][q] != 0.0 for p in range(m) for q in range(p + 1, m)):
            return [T[i][i] for i in range(m)], Y, sweeps
        if sweeps == MAX_SWEEPS:
            return None
        sweeps += 1
        for p in range(m):
            for q in range(p + 1, m):
                a = T[p][q]
                if a == 0.0:
                    continue
                app, aqq = T[p][p], T[q][q]
                if abs(app) + abs(a) == abs(app) and abs(aqq) + abs(a) == abs(aqq):
                    T[p][q] = T[q][p] = 0.0
                    continue
                tau = TK.ieee_div(aqq - app, 2.0 * a)
                den = abs(tau) + _root(1.0 + tau * tau)
                t = TK.ieee_div(1.0 if tau >= 0.0 else -1.0, den)
                c = TK.ieee_div(1.0, _root(1.0 + t * t))
                s = t * c
                for r in range(m):
                    if r == p or r == q:
                        continue
                    rp, rq = T[r][p], T[r][q]
                    T[r][p] = T[p][r] = c * rp - s * rq
                    T[r][q] = T[q][r] = s * rp + c * rq
                T[p][p] = app - t * a
                T[q][q] = aqq + t * a
                T[p][q] = T[q][p] = 0.0
                for r in range(m):
                    rp, rq = Y[r][p], Y[r][q]
                    Y[r][p] = c * rp - s * rq
                    Y[r][q] = s * rp + c * rq


def _root(v):
    if v != v or v < 0.0:
        return float("nan")
    return math.sqrt(v) if v != float("inf") else v


def ordered(theta, which):
    """the columns ordered stably by `which`"""
    key = {0: lambda i: -theta[i], 1: lambda i: theta[i], 2: lambda i: -abs(theta[i])}[which]
    return sorted(range(len(theta)), key=key)


# ---- the solver ------------------------------------------------------------------------------------------------------------
class Inverse(object):
    """OP = (A - sigma I)^-1 by krylov_cases.cg on the shifted operator"""

    def __init__(self, shifted, sigma, M=None, rtol=1e-12, atol=0.0, max_iter=2000):
        self.op = shifted if callable(shifted) else K.RowSerial(shifted)
        self.sigma, self.M, self.rtol, self.atol, self.max_iter = float(sigma), M, rtol, atol, max_iter


class Outcome(object):
    def __init__(self, reason, cycles, ops, values, vectors, residuals, history, inner, sweeps, estimates):
        self.reason, self.cycles, self.ops, self.inner, self.sweeps = reason, cycles, ops, inner, sweeps
        self.values = np.array(values, dtype=np.float64)
        self.vectors = vectors  # n x pairs
        self.residuals = np.array(residuals, dtype=np.float64)
        self.history = np.array(history, dtype=np.float64)
        self.estimates = np.array(estimates, dtype=np.float64)  # est_i of the last close, i < pairs
        self.pairs = len(self.values)

    @property
    def result(self):
        return [self.reason, self.cycles, self.ops, self.pairs, self.inner, self.sweeps]


def eigsh(S, v0, nev, which="LA", ncv=20, tol=1e-10, atol=0.0, max_restarts=1000, inverse=None):
    """the header's sequence on the scipy matrix (or callable operator) S; inverse: an Inverse, or None"""
    A_op = S if callable(S) else K.RowSerial(S)
    cplx = np.iscomplexobj(v0)
    Z = G._Complex if cplx else G._Real
    A = Z.A
    v0 = np.asarray(v0, dtype=A.dtype)
    with np.errstate(all="ignore"):
        return _eigsh(A_op, v0, nev, WHICH[which] if isinstance(which, str) else which, ncv, tol, atol, max_restarts,
                      inverse, Z, A)


def _eigsh(A_op, v0, nev, which, m, tol, atol, max_restarts, inverse, Z, A):
    n = len(v0)
    state = {"ops": 0, "inner": 0, "cycles": 0, "sweeps": 0}
    eta = _root(A.real(A.dot(v0, v0)))
    history = [eta]

    def done(reason, values=(), vectors=None, residuals=(), estimates=()):
        vectors = np.zeros((n, 0), dtype=A.dtype) if vectors is None else vectors
        return Outcome(reason, state["cycles"], state["ops"], values, vectors, residuals, history, state["inner"],
                       state["sweeps"], estimates)

    if not math.isfinite(eta):
        return done(3)
    if eta == 0.0:
        return done(2)
    V = [Z.vector_over(v0, eta)]
    k, theta_kept, s_kept = 0, [], []
    while True:
        invariant = False
        for j in range(k, m):
            if inverse is None:
                w = A_op(V[j])
            else:
                out = K.cg(inverse.op, V[j], inverse.M, None, inverse.rtol, inverse.atol, inverse.max_iter)
                state["inner"] += out.iterations
                if out.reason != 0:
                    return done(4)
                w = out.x
            c1 = [A.dot(V[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = w - A.scaled(c1[i], V[i])
            c2 = [A.dot(V[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = w - A.scaled(c2[i], V[i])
            alpha_j = A.real(Z.add(c1[j], c2[j]))
            eta = _root(A.real(A.dot(w, w)))
            if j == k:
                alpha, beta = [], []
            alpha.append(alpha_j)
            beta.append(eta)
            state["ops"] += 1
            if not (math.isfinite(alpha_j) and math.isfinite(eta)):
                return done(3)
            if eta == 0.0:
                invariant = True
                break
            V.append(Z.vector_over(w, eta))
        mp = k + len(alpha)
        # ---- close
        T = [[0.0] * mp for _ in range(mp)]
        for i in range(k):
            T[i][i] = theta_kept[i]
            T[i][k] = T[k][i] = s_kept[i]
        for j in range(k, mp):
            T[j][j] = alpha[j - k]
            if j < mp - 1:
                T[j][j + 1] = T[j + 1][j] = beta[j - k]
        last = beta[mp - 1 - k]
        solved = jacobi(T)
        if solved is None:
            return done(3)
        theta, Y, sweeps = solved
        if not all(math.isfinite(t) for t in theta) or not all(math.isfinite(y) for row in Y for y in row):
            return done(3)
        state["cycles"] += 1
        state["sweeps"] = max(state["sweeps"], sweeps)
        order = ordered(theta, which)
        pairs = min(nev, mp)
        est = [abs(last * Y[mp - 1][order[i]]) for i in range(mp)]
        history.append(max(est[:pairs]))
        converged = all(est[i] <= max(tol * abs(theta[order[i]]), atol) for i in range(pairs))
        reason = None
        if invariant:
            reason = 0 if mp >= nev else 2
        elif converged:
            reason = 0
        elif state["cycles"] >= max_restarts:
            reason = 1
        basis = np.array(V[:mp]).T
        if reason is not None:
            Yp = np.array([[Y[r][order[i]] for i in range(pairs)] for r in range(mp)], dtype=np.float64)
            X = rotate(basis, Yp)
            values, residuals = [], []
            for i in range(pairs):
                th = theta[order[i]]
                lam = th if inverse is None else inverse.sigma + TK.ieee_div(1.0, th)
                x = np.ascontiguousarray(X[:, i])
                r = A_op(x) - real_times(lam, x)
                values.append(lam)
                residuals.append(_root(A.real(A.dot(r, r))))
            return done(reason, values, X, residuals, est[:pairs])
        # ---- restart
        k = min(mp - 1, nev + (mp - nev) // 2)
        Yk = np.array([[Y[r][order[i]] for i in range(k)] for r in range(mp)], dtype=np.float64)
        kept = rotate(basis, Yk)
        V = [np.ascontiguousarray(kept[:, i]) for i in range(k)] + [V[mp]]
        theta_kept = [theta[order[i]] for i in range(k)]
        s_kept = [last * Y[mp - 1][order[i]] for i in range(k)]


# ---- the committed cases ---------------------------------------------------------------------------------------------------
def start_vector(n, cplx=False):
    """numpy.random.default_rng(0).standard_normal (complex: both parts), the Python layer's default"""
    rng = np.random.default_rng(0)
    if cplx:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex128)
    return rng.standard_normal(n)


def _csr(S):
    S = sp.csr_matrix(S)
    S.sort_indices()
    return S


@functools.lru_cache(maxsize=None)
def matrix(name):
    """the committed matrices; every wanted eigenvalue of a committed case is simple"""
    if name == "ramp":  # tridiag(-1, 2, -1) + diag(linspace(0, 1)), n = 300
        n = 300
        return _csr(sp.diags([-np.ones(n - 1), 2.0 + np.linspace(0.0, 1.0, n), -np.ones(n - 1)], [-1, 0, 1]))
    if name == "hermitian":  # complex Hermitian tridiagonal, n = 200
        n = 200
        rng = np.random.default_rng(7)
        off = rng.uniform(-1.0, 1.0, n - 1) + 1j * rng.uniform(-1.0, 1.0, n - 1)
        return _csr(sp.diags([off.conj(), np.linspace(1.0, 3.0, n).astype(np.complex128), off], [-1, 0, 1]))
    if name == "grid":  # 1.0 L (x) I (x) I + 1.3 I (x) L (x) I + 1.7 I (x) I (x) L on 5 x 6 x 7
        return grid(5, 6, 7)
    if name == "banded":  # n = 4100: a ramp with a few well-separated values at the upper end, and a band
        n = 4100
        d = np.linspace(1.0, 2.0, n)
        d[-6:] = [4.0, 5.5, 7.0, 9.0, 11.5, 14.0]
        return _csr(sp.diags([0.01 * np.ones(n - 3), 0.02 * np.ones(n - 1), d, 0.02 * np.ones(n - 1), 0.01 * np.ones(n - 3)],
                             [-3, -1, 0, 1, 3]))
    if name == "small":  # n = 8, for ncv == n
        return _csr(sp.diags([-np.ones(7), np.arange(1.0, 9.0), -np.ones(7)], [-1, 0, 1]))
    raise KeyError(name)


def laplacian(m):
    return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr")


def grid(a, b, c, weights=(1.0, 1.3, 1.7)):
    """the anisotropic Laplacian as `kronecker` and `lin` assemble it: each term a Kronecker product scaled entry by
    entry, the three added left to right"""
    Ia, Ib, Ic = sp.identity(a, format="csr"), sp.identity(b, format="csr"), sp.identity(c, format="csr")
    terms = (sp.kron(sp.kron(laplacian(a), Ib), Ic), sp.kron(sp.kron(Ia, laplacian(b)), Ic),
             sp.kron(sp.kron(Ia, Ib), laplacian(c)))
    S = _csr(weights[0] * terms[0]) + _csr(weights[1] * terms[1])
    return _csr(_csr(S) + _csr(weights[2] * terms[2]))


def shifted(S, sigma):
    """A - sigma I as `lin` makes it: 1 * a + (-sigma) * 1 on the diagonal, one rounding"""
    S = _csr(S)
    return _csr(S - sigma * sp.identity(S.shape[0], format="csr", dtype=S.dtype))


# (matrix, which, nev, ncv, tol, max_restarts): direct mode, every one a bit test on the device
DIRECT = (("ramp", "LA", 3, 12, 1e-10, 200), ("ramp", "LA", 3, 20, 1e-10, 200), ("ramp", "SA", 3, 12, 1e-10, 200),
          ("ramp", "SA", 3, 20, 1e-10, 200), ("hermitian", "LA", 3, 16, 1e-10, 200), ("hermitian", "SA", 2, 12, 1e-10, 200),
          ("grid", "SA", 4, 20, 1e-10, 200), ("grid", "LM", 3, 16, 1e-10, 200), ("banded", "LA", 4, 12, 1e-8, 50),
          ("small", "LA", 2, 8, 1e-10, 50), ("small", "SA", 3, 4, 1e-10, 200))
# (sigma, preconditioner, nev, ncv): inverse mode on the grid, which = LM, tol 1e-10, inner CG to rtol 1e-12
INVERSE = ((0.0, None, 3, 12), (0.0, "jacobi", 3, 12), (0.0, "amg", 3, 12), (5.0, None, 3, 12), (5.0, "jacobi", 3, 12),
           (5.0, "amg", 3, 12))
INNER_RTOL, INNER_MAXITER = 1e-12, 2000


@functools.lru_cache(maxsize=None)
def reference(name, which, nev, ncv, tol, max_restarts):
    S = matrix(name)
    out = eigsh(S, start_vector(S.shape[0], np.iscomplexobj(S.data)), nev, which, ncv, tol, 0.0, max_restarts)
    for a in (out.values, out.vectors, out.residuals, out.history):
        a.setflags(write=False)
    return out


def inverse_reference(sigma, M, nev, ncv, tol=1e-10, max_restarts=200, max_iter=INNER_MAXITER):
    """M: None, 'jacobi', or a callable preconditioner (the restated AMG cycle on the exported levels)"""
    S = matrix("grid")
    Sh = shifted(S, sigma)
    if M == "jacobi":
        M = K.preconditioner(Sh, "jacobi")
    return eigsh(S, start_vector(S.shape[0]), nev, "LM", ncv, tol, 0.0, max_restarts,
                 Inverse(Sh, sigma, M, INNER_RTOL, 0.0, max_iter))


def norm_inf(S):
    return float(abs(sp.csr_matrix(S)).sum(axis=1).max())


if __name__ == "__main__":  # what every committed case does: checked here, without a GPU
    import time
    for case in DIRECT:
        t0 = time.time()
        out = reference(*case)
        S = matrix(case[0])
        exact = np.linalg.eigvalsh(S.toarray())
        err = max(np.min(np.abs(exact - v)) for v in out.values)
        print("%-9s %s nev %d ncv %2d  reason %-12s cycles %3d  ops %4d  sweeps %2d  residual %.2e  estimate %.2e  "
              "|value - eigvalsh| %.1e  %.2f s" % (case[0], case[1], case[2], case[3], REASONS[out.reason], out.cycles, out.ops,
                                                  out.sweeps, out.residuals.max(), out.estimates.max(), err,
                                                  time.time() - t0))
    for sigma, M, nev, ncv in INVERSE:
        if M == "amg":
            continue  # the cycle is restated on the levels the device exports
        t0 = time.time()
        out = inverse_reference(sigma, M, nev, ncv)
        print("grid sigma %.1f %-6s nev %d ncv %2d  reason %-12s cycles %3d  ops %4d  inner %5d  residual %.2e  values %s  "
              "%.2f s" % (sigma, M, nev, ncv, REASONS[out.reason], out.cycles, out.ops, out.inner, out.residuals.max(),
                          out.values, time.time() - t0))
