"""The yardstick of tests/test_gpu_gmres.py and tests/test_gmres_cpu.py: a serial restatement of the section "restarted
GMRES on handles" of include/sparse_linear_hip.h, built from the pieces of tests/krylov_cases.py (the fold, the
row-serial operator, the two arithmetics, the preconditioner) and the cycle of tests/amg_cases.py.  It never runs code of
the library under test.

Every product, sum, quotient and root is one separately rounded IEEE operation.  A product of two entries is
Data.Complex's (c_mul); a real number times an entry and an entry over a real number are done part by part; vectors over
a real number are divided part by part too (numpy's complex / float is NOT that, so the parts are divided apart).
`python tests/gmres_cases.py` prints what every committed case does, without a GPU."""
import functools
import math

import numpy as np

import krylov_cases as K
import trisolve_cases as TK

REASONS = K.REASONS


# ---- scalars: floats, or (re, im) pairs ----------------------------------------------------------------------------------
class _Real(object):
    A = K.Real

    @staticmethod
    def entry(re):
        return re

    @staticmethod
    def add(a, b):
        return a + b

    @staticmethod
    def sub(a, b):
        return a - b

    @staticmethod
    def conj(a):
        return a

    @staticmethod
    def times(s, a):  # a real number times an entry
        return s * a

    @staticmethod
    def over(a, d):  # an entry over a real number
        return TK.ieee_div(a, d)

    @staticmethod
    def neg(a):
        return -a

    @staticmethod
    def parts(a):
        return a, 0.0

    @staticmethod
    def modulus(a):
        return abs(a)

    @staticmethod
    def vector_over(v, d):
        with np.errstate(all="ignore"):
            return v / d


class _Complex(object):
    A = K.Complex

    @staticmethod
    def entry(re):
        return (re, 0.0)

    @staticmethod
    def add(a, b):
        return (a[0] + b[0], a[1] + b[1])

    @staticmethod
    def sub(a, b):
        return (a[0] - b[0], a[1] - b[1])

    @staticmethod
    def conj(a):
        return (a[0], -a[1])

    @staticmethod
    def times(s, a):
        return (s * a[0], s * a[1])

    @staticmethod
    def over(a, d):
        return (TK.ieee_div(a[0], d), TK.ieee_div(a[1], d))

    @staticmethod
    def neg(a):
        return (-a[0], -a[1])

    @staticmethod
    def parts(a):
        return a

    @staticmethod
    def modulus(a):
        return math.sqrt(a[0] * a[0] + a[1] * a[1])

    @staticmethod
    def vector_over(v, d):
        with np.errstate(all="ignore"):
            return K._cvec(v.real / d, v.imag / d)


def _root(v):
    return math.sqrt(v) if v >= 0.0 else float("nan")


class Outcome(object):
    def __init__(self, x, iterations, reason, cycles, history, residual, spmvs, applications, basis):
        self.x, self.iterations, self.reason, self.cycles = x, iterations, reason, cycles
        self.history = np.array(history, dtype=np.float64)
        self.residual = np.array(residual, dtype=np.float64)
        self.spmvs, self.applications = spmvs, applications
        self.basis = basis  # v_0 ... of the first cycle, as columns (None unless asked for)


def gmres(S, b, M=None, x0=None, restart=30, rtol=1e-8, atol=0.0, max_iter=1000, keep_basis=False):
    """right-preconditioned restarted GMRES with CGS2, the header's sequence"""
    op = S if callable(S) else K.RowSerial(S)
    M = M or K.Preconditioner()
    cplx = np.iscomplexobj(b)
    Z = _Complex if cplx else _Real
    A = Z.A
    b = np.asarray(b, dtype=A.dtype)
    with np.errstate(all="ignore"):
        return _gmres(op, b, M, x0, restart, rtol, atol, max_iter, keep_basis, Z, A)


def _gmres(op, b, M, x0, m, rtol, atol, max_iter, keep_basis, Z, A):
    count = {"spmv": 0, "apply": 0}

    def product(v):
        count["spmv"] += 1
        return op(v)

    def precondition(v):
        if M.none:
            return v
        count["apply"] += 1
        return M(v)

    x = np.zeros(len(b), dtype=A.dtype) if x0 is None else np.array(x0, dtype=A.dtype)
    it, cycles = 0, 0
    history, residual = [], [0.0, 0.0]
    thresh = None
    first_basis = None
    while True:
        # ---- cycle start
        r = b.copy() if (cycles == 0 and x0 is None) else b - product(x)
        rho = A.real(A.dot(r, r))
        residual[0] = _root(rho)
        if thresh is None:
            bb = A.real(A.dot(b, b))
            history.append(_root(rho))
            residual[1] = history[0]
            thresh = K._threshold(rtol, atol, bb) if math.isfinite(bb) else float("nan")
            if not math.isfinite(bb):
                rho = float("nan")  # <b,b> not finite: reason 3 below
        reason = None
        if not math.isfinite(rho):
            reason = 3
        elif math.sqrt(rho) <= thresh:
            reason = 0
        elif it >= max_iter:
            reason = 1
        if reason is not None:
            return Outcome(x, it, reason, cycles, history, residual, count["spmv"], count["apply"], first_basis)
        cycles += 1
        beta = math.sqrt(rho)
        V = [Z.vector_over(r, beta)]
        g = [Z.entry(beta)]
        R = {}  # (row, column)
        cs, sn = [], []
        k, pending = None, None
        for j in range(m):
            w = product(precondition(V[j]))
            c1 = [A.dot(V[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = w - A.scaled(c1[i], V[i])
            c2 = [A.dot(V[i], w) for i in range(j + 1)]
            for i in range(j + 1):
                w = w - A.scaled(c2[i], V[i])
            h = [Z.add(c1[i], c2[i]) for i in range(j + 1)]
            eta = _root(A.real(A.dot(w, w)))
            if not (math.isfinite(eta) and all(A.finite(v) for v in h)):
                k, pending = j, 3
                break
            for i in range(j):
                a, bnext = h[i], h[i + 1]
                h[i] = Z.add(A.mul(Z.conj(cs[i]), a), Z.times(sn[i], bnext))
                h[i + 1] = Z.sub(A.mul(cs[i], bnext), Z.times(sn[i], a))
            re, im = Z.parts(h[j])
            t = math.sqrt(re * re + im * im + eta * eta)
            if t == 0.0:
                k, pending = j, 2
                break
            if not math.isfinite(t):
                k, pending = j, 3
                break
            cs.append(Z.over(h[j], t))
            sn.append(TK.ieee_div(eta, t))
            for i in range(j):
                R[(i, j)] = h[i]
            R[(j, j)] = t
            g.append(Z.neg(Z.times(sn[j], g[j])))
            g[j] = A.mul(Z.conj(cs[j]), g[j])
            it += 1
            history.append(Z.modulus(g[j + 1]))
            if history[it] <= thresh or eta == 0.0 or j + 1 == m or it >= max_iter:
                k = j + 1
                break
            V.append(Z.vector_over(w, eta))
        if keep_basis and first_basis is None:
            first_basis = np.array(V).T
        # ---- close
        if k > 0:
            y = [None] * k
            for i in range(k - 1, -1, -1):
                a = g[i]
                for l in range(i + 1, k):
                    a = Z.sub(a, A.mul(R[(i, l)], y[l]))
                y[i] = Z.over(a, R[(i, i)])
            u = A.scaled(y[0], V[0])
            for l in range(1, k):
                u = u + A.scaled(y[l], V[l])
            x = x + precondition(u)
        residual[1] = history[it]
        if pending is not None:
            return Outcome(x, it, pending, cycles, history, residual, count["spmv"], count["apply"], first_basis)


# ---- the committed cases ---------------------------------------------------------------------------------------------------
# (matrix, preconditioner, restart, max_iter); every one is a bit test on the device
CASES = (("poisson", None, 30, 60), ("poisson", "ilu0", 30, 2000), ("poisson", "sgs", 30, 2000),
         ("shifted", None, 5, 2000), ("shifted", None, 30, 2000), ("shifted", "jacobi", 1, 2000),
         ("shifted", "ilu0", 30, 2000), ("unsym", "jacobi", 5, 2000), ("unsym", "ilu0", 5, 2000),
         ("unsym", None, 30, 45), ("unsymz", "jacobi", 5, 2000), ("unsymz", "sgs", 30, 2000))
# the cases the restatement checks itself on (tests/test_gmres_cpu.py)
SELF_CHECKED = (("shifted", None, 30), ("unsym", "jacobi", 5), ("unsymz", "ilu0", 30), ("poisson", "ilu0", 30))
RTOL = K.RTOL


@functools.lru_cache(maxsize=None)
def reference(name, kind, restart, max_iter=2000, start=False, keep_basis=False):
    """the yardstick's Outcome for a committed case; start: a non-zero x0 (krylov_cases.start_vector)"""
    out = gmres(K._operator(name), K.rhs(name), K._preconditioner(name, kind), K.start_vector(name) if start else None,
                restart, RTOL, 0.0, max_iter, keep_basis)
    out.x.setflags(write=False)
    out.history.setflags(write=False)
    return out


if __name__ == "__main__":  # what every committed case does: checked here, without a GPU
    import time
    for name, kind, restart, max_iter in CASES + tuple(c + (2000,) for c in SELF_CHECKED if c + (2000,) not in CASES):
        t0 = time.time()
        out = reference(name, kind, restart, max_iter)
        print("%-8s %-6s restart %3d  iterations %4d in %3d cycles  reason %-9s  residual %.3e  estimate %.3e  true "
              "relative %.2e  %.2f s" % (name, kind, restart, out.iterations, out.cycles, REASONS[out.reason],
                                         out.residual[0], out.residual[1],
                                         K.true_relative_residual(K.matrix(name), out.x, K.rhs(name)), time.time() - t0))
