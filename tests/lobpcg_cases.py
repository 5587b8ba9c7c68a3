"""The yardstick of tests/test_gpu_lobpcg.py and tests/test_lobpcg_cpu.py: a serial restatement of the section "LOBPCG on
handles" of include/sparse_linear_hip.h, built from the pieces of tests/krylov_cases.py (the fold, the inner product, the
row-serial operator, the preconditioners), tests/gmres_cases.py (the scalars), tests/eigsh_cases.py (the real Jacobi, the
real rotation) and tests/gram_cases.py (the rotation with a complex Y), plus the complex Hermitian Jacobi of the header in
plain Python floats and the method itself.  It never runs code of the library under test.

Every product, sum, quotient and root is one separately rounded IEEE operation.  `python tests/lobpcg_cases.py` prints
reason, iterations, drops and sweeps of every committed case, without a GPU."""
import functools
import math

import numpy as np
import scipy.sparse as sp

import eigsh_cases as EK
import gmres_cases as G
import gram_cases as GK
import krylov_cases as K
import trisolve_cases as TK

REASONS = ("converged", "max_iter", "start_rank_deficient", "non_finite")
LARGEST, SMALLEST = 0, 1  # SPL_EIGSH_largest_algebraic, SPL_EIGSH_smallest_algebraic
MAX_SWEEPS = 60
DROP_RATIO = 2.0 ** -40

_root = EK._root
_div = TK.ieee_div


# ---- the complex Hermitian Jacobi ------------------------------------------------------------------------------------------
def jacobi_hermitian(Tr, Ti):
    """(theta, Yr, Yi, sweeps) of the Hermitian T = Tr + i Ti (lists of lists of floats, changed in place; the diagonal of
    Ti is not read), or None past MAX_SWEEPS.  The rule of the header, operation by operation"""
    m = len(Tr)
    Yr = [[1.0 if r == c else 0.0 for c in range(m)] for r in range(m)]
    Yi = [[0.0] * m for _ in range(m)]
    sweeps = 0
    while True:
        if not any(Tr[p][q] != 0.0 or Ti[p][q] != 0.0 for p in range(m) for q in range(p + 1, m)):
            return [Tr[i][i] for i in range(m)], Yr, Yi, sweeps
        if sweeps == MAX_SWEEPS:
            return None
        sweeps += 1
        for p in range(m):
            for q in range(p + 1, m):
                ar, ai = Tr[p][q], Ti[p][q]
                if ar == 0.0 and ai == 0.0:
                    continue
                g = _root(ar * ar + ai * ai)
                app, aqq = Tr[p][p], Tr[q][q]
                if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                    Tr[p][q] = Tr[q][p] = 0.0
                    Ti[p][q] = Ti[q][p] = 0.0
                    continue
                ur, ui = _div(ar, g), _div(ai, g)
                tau = _div(aqq - app, 2.0 * g)
                den = abs(tau) + _root(1.0 + tau * tau)
                t = _div(1.0 if tau >= 0.0 else -1.0, den)
                c = _div(1.0, _root(1.0 + t * t))
                s = t * c
                for r in range(m):
                    if r == p or r == q:
                        continue
                    pr, pi, xr, xi = Tr[r][p], Ti[r][p], Tr[r][q], Ti[r][q]
                    qr, qi = xr * ur + xi * ui, xi * ur - xr * ui
                    npr, npi = c * pr - s * qr, c * pi - s * qi
                    nqr, nqi = s * pr + c * qr, s * pi + c * qi
                    Tr[r][p], Ti[r][p], Tr[p][r], Ti[p][r] = npr, npi, npr, -npi
                    Tr[r][q], Ti[r][q], Tr[q][r], Ti[q][r] = nqr, nqi, nqr, -nqi
                Tr[p][p] = app - t * g
                Tr[q][q] = aqq + t * g
                Tr[p][q] = Tr[q][p] = 0.0
                Ti[p][q] = Ti[q][p] = 0.0
                for r in range(m):
                    pr, pi, xr, xi = Yr[r][p], Yi[r][p], Yr[r][q], Yi[r][q]
                    qr, qi = xr * ur + xi * ui, xi * ur - xr * ui
                    Yr[r][p], Yi[r][p] = c * pr - s * qr, c * pi - s * qi
                    Yr[r][q], Yi[r][q] = s * pr + c * qr, s * pi + c * qi


def _finite(values):
    return all(math.isfinite(v) for v in values)


# ---- the method --------------------------------------------------------------------------------------------------------------
class Outcome(object):
    def __init__(self, reason, iterations, spmv_columns, applications, sweeps, dropped, syncs, values, vectors, residuals,
                 history):
        self.reason, self.iterations, self.spmv_columns, self.applications = reason, iterations, spmv_columns, applications
        self.sweeps, self.dropped, self.syncs = sweeps, dropped, syncs
        self.values = np.array(values, dtype=np.float64)
        self.vectors = vectors  # n x pairs
        self.residuals = np.array(residuals, dtype=np.float64)
        self.history = np.array(history, dtype=np.float64)
        self.pairs = len(self.values)

    @property
    def result(self):
        return [self.reason, self.iterations, self.spmv_columns, self.pairs, self.applications, self.sweeps, self.dropped,
                self.syncs]


def lobpcg(S, X0, nev, which=SMALLEST, tol=1e-8, atol=0.0, max_iter=200, M=None):
    """the header's sequence on the scipy matrix (or callable operator) S from the start block X0 (n x block); M: None
    or a callable r -> M^-1 r"""
    A_op = S if callable(S) else K.RowSerial(S)
    X0 = np.asarray(X0)
    cplx = np.iscomplexobj(X0)
    Z = G._Complex if cplx else G._Real
    with np.errstate(all="ignore"):
        return _lobpcg(A_op, X0.astype(Z.A.dtype), nev, which, tol, atol, max_iter, M, Z, Z.A, cplx)


def _lobpcg(A_op, X0, nev, which, tol, atol, max_iter, M, Z, A, cplx):
    n, b = X0.shape
    st = {"it": 0, "spmv": 0, "apps": 0, "sweeps": 0, "dropped": 0, "syncs": 0}
    history = []
    zero = np.zeros(n, dtype=A.dtype)
    cols = [np.ascontiguousarray(X0[:, j]) for j in range(b)] + [zero.copy() for _ in range(2 * b)]
    image = [zero.copy() for _ in range(3 * b)]
    flags = [0] * (3 * b)
    theta = [0.0] * b

    def done(reason, values=(), vectors=None, residuals=()):
        vectors = np.zeros((n, 0), dtype=A.dtype) if vectors is None else vectors
        return Outcome(reason, st["it"], st["spmv"], st["apps"], st["sweeps"], st["dropped"], st["syncs"], values, vectors,
                       residuals, history)

    def norm(v):
        return _root(A.real(A.dot(v, v)))

    def settle(c, with_image=False):
        w = cols[c]
        eta0 = norm(w)
        passes = []
        if c > 0:
            for _ in range(2):
                coef = [A.dot(cols[i], w) for i in range(c)]
                passes.append(coef)
                for i in range(c):
                    w = w - A.scaled(coef[i], cols[i])
        eta2 = norm(w)
        if not (math.isfinite(eta0) and math.isfinite(eta2)):
            flags[c] = 2
        elif eta2 == 0.0 or eta2 <= DROP_RATIO * eta0:
            flags[c] = 1
        else:
            flags[c] = 0
        cols[c] = zero.copy() if flags[c] else Z.vector_over(w, eta2)
        if with_image:  # A x_c receives the same coefficients, the same division and the same zeros
            v = image[c]
            for coef in passes:
                for i in range(c):
                    v = v - A.scaled(coef[i], image[i])
            image[c] = zero.copy() if flags[c] else Z.vector_over(v, eta2)

    def close(mc, kout, count_from):
        """None: go on; else the reason that ends the solve"""
        st["syncs"] += 1
        kept = []
        for j in range(mc):
            if flags[j] == 2 or (j < b and flags[j] != 0):
                return 3
            if flags[j] == 0:
                kept.append(j)
            elif j >= count_from:
                st["dropped"] += 1
        mp = len(kept)
        Tr = [[0.0] * mp for _ in range(mp)]
        Ti = [[0.0] * mp for _ in range(mp)]
        for a in range(mp):
            for c in range(a, mp):
                g = A.dot(cols[kept[a]], image[kept[c]])
                gr, gi = (g[0], 0.0 if a == c else g[1]) if cplx else (g, 0.0)
                if not (math.isfinite(gr) and math.isfinite(gi)):
                    return 3
                Tr[a][c] = Tr[c][a] = gr
                Ti[a][c] = gi
                Ti[c][a] = 0.0 if a == c else -gi
        if cplx:
            solved = jacobi_hermitian(Tr, Ti)
            if solved is None:
                return 3
            values, Yr, Yi, sweeps = solved
        else:
            solved = EK.jacobi(Tr)
            if solved is None:
                return 3
            values, Yr, sweeps = solved
            Yi = [[0.0] * mp for _ in range(mp)]
        if not _finite(values) or not all(_finite(row) for row in Yr) or not all(_finite(row) for row in Yi):
            return 3
        st["sweeps"] = max(st["sweeps"], sweeps)
        order = EK.ordered(values, which)
        Zm = np.zeros((mc, kout), dtype=A.dtype)
        for i in range(kout):
            col = order[i if i < b else i - b]
            for a in range(mp):
                if i >= b and kept[a] < b:
                    continue
                Zm[kept[a], i] = complex(Yr[a][col], Yi[a][col]) if cplx else Yr[a][col]
        rotate = GK.rotate_z if cplx else EK.rotate
        new_s = rotate(np.stack(cols[:mc], axis=1), Zm)
        new_i = rotate(np.stack(image[:mc], axis=1), Zm)
        for i in range(kout):
            cols[i] = np.ascontiguousarray(new_s[:, i])
            image[i] = np.ascontiguousarray(new_i[:, i])
        for i in range(b):
            theta[i] = values[order[i]]
        for j in range(b):  # X' is settled again, A X' with it
            settle(j, True)
        return None

    def finish(reason):
        values, residuals = [], []
        for i in range(nev):
            r = A_op(cols[i]) - EK.real_times(theta[i], cols[i])
            st["spmv"] += 1
            values.append(theta[i])
            residuals.append(norm(r))
        st["syncs"] += 1
        return done(reason, values, np.stack(cols[:nev], axis=1), residuals)

    # ---- start
    for j in range(b):
        settle(j)
    st["syncs"] += 1
    if any(flags[j] == 2 for j in range(b)):
        return done(3)
    if any(flags[j] == 1 for j in range(b)):
        return done(2)
    for j in range(b):
        image[j] = A_op(cols[j])
    st["spmv"] += b
    reason = close(b, b, b)
    if reason is not None:
        return done(reason)
    it = 0
    while True:
        st["it"] = it
        R = [image[i] - EK.real_times(theta[i], cols[i]) for i in range(b)]
        rho = [norm(r) for r in R]
        st["syncs"] += 1
        if not _finite(rho):
            return done(3)
        worst = 0.0
        for i in range(nev):
            if rho[i] > worst:
                worst = rho[i]
        history.append(worst)
        if all(rho[i] <= max(tol * abs(theta[i]), atol) for i in range(nev)):
            return finish(0)
        if it >= max_iter:
            return finish(1)
        for i in range(b):
            if M is None:
                cols[2 * b + i] = R[i]
            else:
                cols[2 * b + i] = np.ascontiguousarray(M(R[i]))
                st["apps"] += 1
        for c in range(b, 3 * b):
            settle(c)
        for c in range(b, 3 * b):
            image[c] = A_op(cols[c])
        st["spmv"] += 2 * b
        reason = close(3 * b, 2 * b, 2 * b if it == 0 else b)
        st["it"] = it + 1
        if reason is not None:
            return done(reason)
        it += 1


# ---- the committed cases ---------------------------------------------------------------------------------------------------
def _csr(S):
    S = sp.csr_matrix(S)
    S.sort_indices()
    return S


def poisson2d(m):
    L, I = EK.laplacian(m), sp.identity(m, format="csr")
    return _csr(sp.kron(L, I) + sp.kron(I, L))


def poisson3d(m):
    L, I = EK.laplacian(m), sp.identity(m, format="csr")
    return _csr(sp.kron(sp.kron(L, I), I) + sp.kron(sp.kron(I, L), I) + sp.kron(sp.kron(I, I), L))


def phased(S, seed=17):
    """D S D^H with a unit-modulus complex diagonal D, part by part: a (x_i x_j + y_i y_j) + i a (y_i x_j - x_i y_j),
    which is Hermitian bit for bit; the entries of S are 4 and -1, so the scaling is exact"""
    S = sp.coo_matrix(S)
    phi = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, S.shape[0])
    x, y = np.cos(phi), np.sin(phi)
    i, j, a = S.row, S.col, S.data
    vals = np.empty(len(a), dtype=np.complex128)
    vals.real = a * (x[i] * x[j] + y[i] * y[j])
    vals.imag = a * (y[i] * x[j] - x[i] * y[j])
    return _csr(sp.coo_matrix((vals, (i, j)), shape=S.shape))


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "poisson12":  # isotropic: lambda_2 is double
        return poisson2d(12)
    if name == "phased12":  # the same spectrum, complex Hermitian
        return phased(poisson2d(12))
    if name == "five":
        return _csr(sp.diags([-np.ones(4), np.array([2.0, 3.0, 4.0, 5.0, 6.0]), -np.ones(4)], [-1, 0, 1]))
    if name == "two":
        return _csr(np.array([[2.0, -1.0], [-1.0, 3.0]]))
    if name == "diagonal":
        return _csr(sp.diags([np.arange(1.0, 9.0)], [0]))
    if name == "grid70":  # n = 4900: more than one chunk of the fold
        return poisson2d(70)
    if name == "poisson8":  # 8^3 = 512 rows, for the preconditioners
        return poisson3d(8)
    raise KeyError(name)


def start_block(n, block, cplx=False, seed=0):
    rng = np.random.default_rng(seed + 1000 * block + n)
    X = rng.standard_normal((n, block))
    if cplx:
        X = X + 1j * rng.standard_normal((n, block))
    return X


# (matrix, block, nev, which, tol, max_iter): every one a bit test on the device; all but the last reach reason 0
CASES = (("poisson12", 6, 4, SMALLEST, 1e-9, 200), ("phased12", 6, 4, SMALLEST, 1e-9, 200),
         ("poisson12", 4, 2, LARGEST, 1e-9, 200), ("five", 2, 2, SMALLEST, 1e-10, 50), ("two", 1, 1, SMALLEST, 1e-10, 50),
         ("grid70", 4, 2, SMALLEST, 1e-9, 3))
# (preconditioner, block, nev, tol, max_iter) on poisson8, smallest; "amg" is restated on the levels the device exports
PRECONDITIONED = (("jacobi", 4, 3, 1e-8, 200), ("sgs", 4, 3, 1e-8, 200), ("ilu0", 4, 3, 1e-8, 200), ("amg", 4, 3, 1e-8, 200))


def start_of(name, block):
    S = matrix(name)
    return start_block(S.shape[0], block, np.iscomplexobj(S.data))


@functools.lru_cache(maxsize=None)
def reference(name, block, nev, which, tol, max_iter, kind=None):
    S = matrix(name)
    M = None if kind is None else K.preconditioner(S, kind)
    out = lobpcg(S, start_of(name, block), nev, which, tol, 0.0, max_iter, M)
    for a in (out.values, out.vectors, out.residuals, out.history):
        a.setflags(write=False)
    return out


def norm_one(S):
    return float(abs(sp.csr_matrix(S)).sum(axis=0).max())


if __name__ == "__main__":  # what every committed case does: checked here, without a GPU
    import time

    def show(label, out, t0):
        print("%-22s reason %-20s iterations %3d  drops %3d  sweeps %2d  spmv columns %4d  applications %4d  residual %.2e"
              "  |X^H X - I| %.1e  %.2f s" % (label, REASONS[out.reason], out.iterations, out.dropped, out.sweeps,
                                            out.spmv_columns, out.applications,
                                            out.residuals.max() if out.pairs else float("nan"),
                                            np.abs(out.vectors.conj().T @ out.vectors - np.eye(out.pairs)).max()
                                            if out.pairs else float("nan"), time.time() - t0))

    for case in CASES:
        t0 = time.time()
        show("%s b%d nev%d w%d" % case[:4], reference(*case), t0)
    for kind, block, nev, tol, max_iter in PRECONDITIONED:
        if kind == "amg":
            continue
        t0 = time.time()
        show("poisson8 %s" % kind, reference("poisson8", block, nev, SMALLEST, tol, max_iter, kind), t0)
