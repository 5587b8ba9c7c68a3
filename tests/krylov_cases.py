"""Inputs and the yardstick of tests/test_gpu_krylov.py and tests/test_krylov_cpu.py.

The yardstick restates the section "fixed-order inner product, preconditioned CG and BiCGSTAB" of
include/sparse_linear_hip.h on the CPU:

  * fold: the chunks of 4096 entries are reshaped to 16 x 256, the 16 steps of every lane run as a loop over the rows
    (a short chunk is padded with +0.0, which changes no sum: a lane's sum starts from +0.0 and can never be -0.0), and
    the tree s[t] += s[t + h] is done by halving; the partials are folded again until one value is left;
  * the operator: the row-serial product, y_r = 0, y_r = y_r + a_rj * x_j in ascending column order, done for all rows
    at once position by position;
  * the preconditioner: the serial substitution loop of tests/trisolve_cases.py for T1 and T2, an entry-wise product
    for the middle part, the ILU(0) values of tests/ilu0_cases.py;
  * the scalars: Python floats, ieee_div / c_mul / c_div of tests/trisolve_cases.py;
  * the vector updates: one numpy product and one numpy sum per entry, complex ones by their parts.

Every product, sum and quotient is one separately rounded IEEE operation (numpy fuses nothing across two ufunc calls).
`python tests/krylov_cases.py` prints what every committed case does, without a GPU."""
import functools
import math

import numpy as np
import scipy.sparse as sp

import ilu0_cases as IK
import trisolve_cases as TK

CHUNK, LANES = 4096, 256
REASONS = ("converged", "max_iter", "breakdown", "non_finite")


# ---- the fold ----------------------------------------------------------------------------------------------------------
def fold_levels(length):
    """the levels of the header: two up to 4096^2 entries, three beyond"""
    return 2 if length <= CHUNK * CHUNK else 3


def fold(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    if len(v) == 0:
        return 0.0
    while True:
        nchunks = -(-len(v) // CHUNK)
        padded = np.zeros(nchunks * CHUNK)
        padded[:len(v)] = v
        rows = padded.reshape(nchunks, CHUNK // LANES, LANES)
        s = np.zeros((nchunks, LANES))
        for k in range(CHUNK // LANES):  # lane t adds the entries t, t + 256, ... in ascending order
            s = s + rows[:, k, :]
        h = LANES // 2
        while h >= 1:
            s[:, :h] = s[:, :h] + s[:, h:2 * h]
            h //= 2
        v = np.ascontiguousarray(s[:, 0])
        if len(v) == 1:
            return float(v[0])


def _cvec(re, im):
    out = np.empty(len(re), dtype=np.complex128)
    out.real = re
    out.imag = im
    return out


# ---- the two arithmetics: vectors are float64 / complex128 arrays, scalars floats / (re, im) pairs --------------------
class Real(object):
    cplx = False
    dtype = np.float64
    zero = 0.0

    @staticmethod
    def products(a, b):
        return (a * b,)

    @staticmethod
    def dot(a, b):
        return fold(a * b)

    @staticmethod
    def scaled(s, v):  # s v
        return s * v

    @staticmethod
    def entrywise(d, v):
        return d * v

    @staticmethod
    def div(a, b):
        return TK.ieee_div(a, b)

    @staticmethod
    def mul(a, b):
        return a * b

    @staticmethod
    def is_zero(a):
        return a == 0.0

    @staticmethod
    def finite(a):
        return math.isfinite(a)

    @staticmethod
    def real(a):
        return a


class Complex(object):
    cplx = True
    dtype = np.complex128
    zero = (0.0, 0.0)

    @staticmethod
    def products(a, b):
        """conj(a_i) * b_i by Data.Complex's product on (a_re, -a_im) and b"""
        ar, ai, br, bi = a.real, -a.imag, b.real, b.imag
        return ar * br - ai * bi, ar * bi + ai * br

    @classmethod
    def dot(cls, a, b):
        re, im = cls.products(a, b)
        return fold(re), fold(im)

    @staticmethod
    def scaled(s, v):
        sr, si = s
        return _cvec(sr * v.real - si * v.imag, sr * v.imag + si * v.real)

    @staticmethod
    def entrywise(d, v):
        return _cvec(d.real * v.real - d.imag * v.imag, d.real * v.imag + d.imag * v.real)

    @staticmethod
    def div(a, b):
        return TK.c_div(a[0], a[1], b[0], b[1])

    @staticmethod
    def mul(a, b):
        return TK.c_mul(a[0], a[1], b[0], b[1])

    @staticmethod
    def is_zero(a):
        return a[0] == 0.0 and a[1] == 0.0

    @staticmethod
    def finite(a):
        return math.isfinite(a[0]) and math.isfinite(a[1])

    @staticmethod
    def real(a):
        return a[0]


def arithmetic(cplx):
    return Complex if cplx else Real


def dot(a, b):
    """<a,b> as the device computes it: a float, or a complex"""
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a):
        re, im = Complex.dot(a, b)
        return complex(re, im)
    return Real.dot(a, b)


# ---- the operator ------------------------------------------------------------------------------------------------------
class RowSerial(object):
    """y = A x with every row's sum in ascending column order, from +0.0, all rows at once position by position"""

    def __init__(self, S):
        S = sp.csr_matrix(S)
        S.sort_indices()
        self.S = S
        self.n = S.shape[0]
        self.A = arithmetic(np.iscomplexobj(S.data))
        lens = np.diff(S.indptr)
        self.steps = []
        for k in range(int(lens.max()) if self.n else 0):
            rows = np.nonzero(lens > k)[0]
            q = S.indptr[rows] + k
            self.steps.append((rows, S.data[q], S.indices[q]))

    def __call__(self, x):
        y = np.zeros(self.n, dtype=self.A.dtype)
        for rows, vals, cols in self.steps:
            y[rows] = y[rows] + self.A.entrywise(vals, x[cols])
        return y


# ---- the preconditioner ------------------------------------------------------------------------------------------------
class Preconditioner(object):
    """z = T2^-1 (mid (.) (T1^-1 r)); a part is (scipy matrix, lower, unit) or None, mid an array or None"""

    def __init__(self, T1=None, mid=None, T2=None):
        self.tri = [None if t is None else (TK.take_triangle(t[0], t[1]), t[2]) for t in (T1, T2)]
        self.mid = mid
        self.none = T1 is None and mid is None and T2 is None

    @staticmethod
    def _solve(tri, v):
        T, unit = tri
        if T.cplx:
            x = TK.serial_solve(T, unit, list(zip(v.real.tolist(), v.imag.tolist())))
            return _cvec([p[0] for p in x], [p[1] for p in x])
        return np.array(TK.serial_solve(T, unit, v.tolist()), dtype=np.float64)

    def __call__(self, r):
        v = r
        if self.tri[0] is not None:
            v = self._solve(self.tri[0], v)
        if self.mid is not None:
            v = arithmetic(np.iscomplexobj(r)).entrywise(self.mid, v)
        if self.tri[1] is not None:
            v = self._solve(self.tri[1], v)
        return v


def reciprocal_diagonal(S):
    """1 / a_ii: the IEEE quotient, Data.Complex's scaled one on complex values"""
    d = sp.csr_matrix(S).diagonal()
    if np.iscomplexobj(d):
        q = [TK.c_div(1.0, 0.0, re, im) for re, im in zip(d.real.tolist(), d.imag.tolist())]
        return _cvec([p[0] for p in q], [p[1] for p in q])
    return np.array([TK.ieee_div(1.0, v) for v in d.tolist()], dtype=np.float64)


def preconditioner(S, kind, mid=None):
    """the yardstick's preconditioner of the scipy matrix S: None, 'jacobi', 'sgs' or 'ilu0'; mid: the middle part the
    device was given, where the test did not make it by reciprocal_diagonal / the diagonal itself"""
    S = sp.csr_matrix(S)
    if kind is None:
        return Preconditioner()
    if kind == "jacobi":
        return Preconditioner(None, reciprocal_diagonal(S) if mid is None else mid, None)
    if kind == "sgs":
        return Preconditioner((S, True, False), S.diagonal() if mid is None else mid, (S, False, False))
    if kind == "ilu0":
        F = sp.csr_matrix((IK.serial_ilu0(S), S.indices, S.indptr), shape=S.shape)
        return Preconditioner((F, True, True), None, (F, False, False))
    raise KeyError(kind)


# ---- the drivers -------------------------------------------------------------------------------------------------------
class Outcome(object):
    def __init__(self, x, iterations, reason, history):
        self.x, self.iterations, self.reason = x, iterations, reason
        self.history = np.array(history, dtype=np.float64)


def _threshold(rtol, atol, bb):
    scaled = rtol * math.sqrt(bb)
    return scaled if scaled > atol else atol


def _start(A, op, b, x0):
    if x0 is None:
        x, r = np.zeros(len(b), dtype=A.dtype), b.copy()
    else:
        x = np.array(x0, dtype=A.dtype)
        r = b - op(x)
    return x, r


def _first_checks(rr, bb, thresh, max_iter):
    if not (math.isfinite(rr) and math.isfinite(bb)):
        return 3
    if math.sqrt(rr) <= thresh:
        return 0
    if max_iter <= 0:
        return 1
    return None


def _residual_checks(rr, thresh, it, max_iter):
    if not math.isfinite(rr):
        return 3
    if math.sqrt(rr) <= thresh:
        return 0
    if it >= max_iter:
        return 1
    return None


def _root(v):
    return math.sqrt(v) if v >= 0.0 else float("nan")


def cg(S, b, M=None, x0=None, rtol=1e-8, atol=0.0, max_iter=1000):
    """standard preconditioned CG, the header's sequence"""
    op = S if callable(S) else RowSerial(S)
    M = M or Preconditioner()
    A = arithmetic(np.iscomplexobj(b))
    x, r = _start(A, op, b, x0)
    rr, bb = A.real(A.dot(r, r)), A.real(A.dot(b, b))
    thresh = _threshold(rtol, atol, bb) if math.isfinite(bb) else float("nan")
    history, it = [_root(rr)], 0
    reason = _first_checks(rr, bb, thresh, max_iter)
    if reason is not None:
        return Outcome(x, it, reason, history)
    z = r if M.none else M(r)
    rho = A.dot(r, z)
    if A.is_zero(rho) or not A.finite(rho):
        return Outcome(x, it, 2, history)
    p = z.copy()
    while True:
        q = op(p)
        d = A.dot(p, q)
        if A.is_zero(d) or not A.finite(d):
            return Outcome(x, it, 2, history)
        alpha = A.div(rho, d)
        x = x + A.scaled(alpha, p)
        r = r - A.scaled(alpha, q)
        rr = A.real(A.dot(r, r))
        it += 1
        history.append(_root(rr))
        reason = _residual_checks(rr, thresh, it, max_iter)
        if reason is not None:
            return Outcome(x, it, reason, history)
        z = r if M.none else M(r)
        new = A.dot(r, z)
        if A.is_zero(new) or not A.finite(new):
            return Outcome(x, it, 2, history)
        beta = A.div(new, rho)
        rho = new
        p = z + A.scaled(beta, p)


def bicgstab(S, b, M=None, x0=None, rtol=1e-8, atol=0.0, max_iter=1000):
    """van der Vorst's BiCGSTAB, preconditioned from the right, the header's sequence"""
    op = S if callable(S) else RowSerial(S)
    M = M or Preconditioner()
    A = arithmetic(np.iscomplexobj(b))
    x, r = _start(A, op, b, x0)
    rhat = r.copy()
    rr, bb = A.real(A.dot(r, r)), A.real(A.dot(b, b))
    thresh = _threshold(rtol, atol, bb) if math.isfinite(bb) else float("nan")
    history, it = [_root(rr)], 0
    reason = _first_checks(rr, bb, thresh, max_iter)
    if reason is not None:
        return Outcome(x, it, reason, history)
    rho = alpha = omega = None
    p = v = None
    while True:
        new = A.dot(rhat, r)
        if A.is_zero(new) or not A.finite(new):
            return Outcome(x, it, 2, history)
        if rho is None:
            p = r.copy()
        else:
            beta = A.mul(A.div(new, rho), A.div(alpha, omega))
            p = r + A.scaled(beta, p - A.scaled(omega, v))
        rho = new
        y = p if M.none else M(p)
        v = op(y)
        d = A.dot(rhat, v)
        if A.is_zero(d) or not A.finite(d):
            return Outcome(x, it, 2, history)
        alpha = A.div(rho, d)
        s = r - A.scaled(alpha, v)
        x = x + A.scaled(alpha, y)
        ss = A.real(A.dot(s, s))
        if not math.isfinite(ss):
            return Outcome(x, it, 3, history)
        if math.sqrt(ss) <= thresh:
            it += 1
            history.append(math.sqrt(ss))
            return Outcome(x, it, 0, history)
        z = s if M.none else M(s)
        t = op(z)
        ts, tt = A.dot(t, s), A.dot(t, t)
        if A.is_zero(tt) or not A.finite(tt):
            return Outcome(x, it, 2, history)
        omega = A.div(ts, tt)
        if A.is_zero(omega) or not A.finite(omega):
            return Outcome(x, it, 2, history)
        x = x + A.scaled(omega, z)
        r = s - A.scaled(omega, t)
        rr = A.real(A.dot(r, r))
        it += 1
        history.append(_root(rr))
        reason = _residual_checks(rr, thresh, it, max_iter)
        if reason is not None:
            return Outcome(x, it, reason, history)


DRIVERS = {"cg": cg, "bicgstab": bicgstab}


# ---- matrices ----------------------------------------------------------------------------------------------------------
GRID = 91  # 8281 unknowns: three chunks, the last of 89 entries


def _neighbours(m):
    i = np.arange(m * m)
    west, east, south, north = i[i % m != 0], i[i % m != m - 1], i[i >= m], i[i < m * m - m]
    return np.concatenate([west, east, south, north]), np.concatenate([west - 1, east + 1, south - m, north + m])


@functools.lru_cache(maxsize=None)
def matrix(name):
    """scipy CSR with sorted indices.
    poisson:     the 5-point Laplacian on a 91 x 91 grid, 4 and -1: symmetric positive definite
    hermitian:   the same pattern, 4.5 on the diagonal and -1 + 0.3i above / -1 - 0.3i below it: Hermitian and strictly
                 dominant (4 |-1 + 0.3i| = 4.18 < 4.5), so positive definite
    shifted:     the Laplacian + (0.5 + 0.5i) I: complex symmetric, not Hermitian
    unsym / unsymz: n = 300, rows of 1 ... 40 entries with the diagonal, unsymmetric, strictly dominant
    poisson3d:   the 7-point Laplacian on 30^3"""
    if name in ("poisson", "hermitian", "shifted"):
        m = GRID
        n = m * m
        r, c = _neighbours(m)
        if name == "poisson":
            return IK.laplacian(m)
        if name == "hermitian":
            v = np.where(c > r, -1.0 + 0.3j, -1.0 - 0.3j)
            d = np.full(n, 4.5 + 0.0j)
        else:
            v = np.full(len(r), -1.0 + 0.0j)
            d = np.full(n, 4.5 + 0.5j)
        S = sp.csr_matrix((np.concatenate([v, d]), (np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)]))),
                          shape=(n, n))
        S.sort_indices()
        return S
    if name in ("unsym", "unsymz"):
        cplx = name == "unsymz"
        rng = np.random.default_rng(77 + cplx)
        n = 300
        want = rng.integers(1, 41, n)
        want[:4] = (1, 2, 40, 39)
        rows, cols = [], []
        for i in range(n):
            others = np.setdiff1d(np.arange(n), [i])
            pick = rng.choice(others, int(want[i]) - 1, replace=False)
            cols.append(pick)
            rows.append(np.full(len(pick), i))
        r, c = np.concatenate(rows), np.concatenate(cols)
        v = rng.uniform(-1.0, 1.0, len(r))
        if cplx:
            v = v + 1j * rng.uniform(-1.0, 1.0, len(r))
        rowsum = np.bincount(r, weights=np.abs(v), minlength=n)
        d = rng.choice([-1.0, 1.0], n) * (1.0 + 1.5 * rowsum)
        if cplx:
            d = d + 0.5j * d
        S = sp.csr_matrix((np.concatenate([v, d]), (np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)]))),
                          shape=(n, n))
        S.sort_indices()
        assert S.nnz == len(v) + n
        return S
    if name == "poisson3d":
        m = 30
        T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
        I = sp.identity(m)
        S = sp.csr_matrix(sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T))
        S.sort_indices()
        return S
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def rhs(name, seed=3):
    S = matrix(name)
    rng = np.random.default_rng(1000 * seed + S.shape[0])
    b = rng.uniform(-1.0, 1.0, S.shape[0])
    if np.iscomplexobj(S.data):
        b = b + 1j * rng.uniform(-1.0, 1.0, S.shape[0])
    b.setflags(write=False)
    return b


# the committed driver cases: (method, matrix); every one runs with every preconditioner
CASES = (("cg", "poisson"), ("cg", "hermitian"), ("bicgstab", "poisson"), ("bicgstab", "shifted"), ("bicgstab", "unsym"),
         ("bicgstab", "unsymz"))
PRECONDITIONERS = (None, "jacobi", "sgs", "ilu0")
RTOL = 1e-8


@functools.lru_cache(maxsize=None)
def _operator(name):
    return RowSerial(matrix(name))


@functools.lru_cache(maxsize=None)
def _preconditioner(name, kind):
    return preconditioner(matrix(name), kind)


@functools.lru_cache(maxsize=None)
def reference(method, name, kind, start=False, max_iter=2000, rtol=RTOL):
    """the yardstick's Outcome for a committed case; start: a non-zero x0 (start_vector)"""
    out = DRIVERS[method](_operator(name), rhs(name), _preconditioner(name, kind), start_vector(name) if start else None,
                          rtol, 0.0, max_iter)
    out.x.setflags(write=False)
    out.history.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def start_vector(name):
    x0 = np.array(rhs(name, seed=9)) * 0.5
    x0.setflags(write=False)
    return x0


def true_relative_residual(S, x, b):
    """|b - A x| / |b| by scipy's product and numpy's norms: independent of the restated sums"""
    return float(np.linalg.norm(b - sp.csr_matrix(S) @ x) / np.linalg.norm(b))


def dot_inputs(n, cplx, seed=1):
    """two vectors of n entries whose products cancel: b = +-a in runs, so partial sums swing through zero, on top of
    values spread over twelve orders of magnitude"""
    rng = np.random.default_rng(4000 + 7 * seed + (n % 9973) + (500 if cplx else 0))
    def one():
        v = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-6, 7, n)
        return v + 1j * rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-6, 7, n) if cplx else v
    a = one()
    sign = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    b = np.where(rng.random(n) < 0.7, sign * a, one())
    return a, b


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


if __name__ == "__main__":  # what every committed case does: checked here, without a GPU
    import time
    for method, name in CASES:
        for kind in PRECONDITIONERS:
            t0 = time.time()
            out = reference(method, name, kind)
            print("%-8s %-9s %-6s iterations %4d reason %-9s true residual %.2e  %.2f s"
                  % (method, name, kind, out.iterations, REASONS[out.reason],
                     true_relative_residual(matrix(name), out.x, rhs(name)), time.time() - t0))
