"""Inputs and the yardstick of tests/test_gpu_amg.py and tests/test_amg_cpu.py.

The yardstick restates the section "aggregation AMG on handles" of include/sparse_linear_hip.h on the CPU:

  * the aggregation, twice, in Python integers on the graph and the priority of tests/coloring_cases.py: `greedy` walks
    the vertices in priority order, an undecided vertex becomes a root and every undecided vertex within distance <= 2
    of it is out; `rounds` simulates the launches, where every undecided vertex that precedes all other vertices within
    distance <= 2 that were undecided when the round began becomes a root, and then every undecided vertex within
    distance <= 2 of a new root is out.  The two must agree (tests/test_amg_cpu.py), and the device must give both;
  * the aggregates: aggregate k is rooted at the k-th root in ascending index; the neighbours of a root join it
    (phase 1); every remaining vertex takes the aggregate of that phase-1 neighbour which precedes the others (phase 2);
  * the cycle: a callable with `.none = False` that tests/krylov_cases.py's drivers take as M, built on
    krylov_cases.RowSerial and krylov_cases.arithmetic: one difference, one product and one sum per entry, each rounded
    once, the products with the matrices row-serial in ascending column order;
  * a scipy hierarchy builder for the checks that need no bits.

`python tests/amg_cases.py` prints the levels and the iteration counts of every committed case, without a GPU."""
import functools

import numpy as np
import scipy.sparse as sp

import coloring_cases as CC
import krylov_cases as K
import trisolve_cases as TK

SEEDS = CC.SEEDS
DEFAULTS = dict(seed=0, sweeps=1, coarse_size=256, max_levels=16, coarse_sweeps=4, plain=False)


# ---- the aggregation ---------------------------------------------------------------------------------------------------
def _precedes(h, u, v):
    return h[u] > h[v] or (h[u] == h[v] and u < v)


def _within_two(adj, v):
    """the vertices within distance <= 2 of v, v itself left out; paths run through any vertex"""
    near = set(adj[v])
    for u in adj[v]:
        near.update(adj[u])
    near.discard(v)
    return near


def greedy_roots(adj, seed):
    """the roots of the serial walk in priority order, ascending"""
    n = len(adj)
    h = [CC.priority(v, seed) for v in range(n)]
    order = sorted(range(n), key=lambda v: (-h[v], v))
    state = [0] * n  # 0 undecided, 1 root, 2 out
    for v in order:
        if state[v]:
            continue
        state[v] = 1
        for u in _within_two(adj, v):
            if state[u] == 0:
                state[u] = 2
    return [v for v in range(n) if state[v] == 1]


def round_roots(adj, seed):
    """(roots ascending, number of rounds) of the simulated launches"""
    n = len(adj)
    h = [CC.priority(v, seed) for v in range(n)]
    near = [_within_two(adj, v) for v in range(n)]
    state = [0] * n
    undecided = list(range(n))
    count = 0
    while undecided:
        count += 1
        fresh = [v for v in undecided if all(state[u] != 0 or _precedes(h, v, u) for u in near[v])]  # the round's start
        for v in fresh:
            state[v] = 1
        for v in fresh:
            for u in near[v]:
                if state[u] == 0:
                    state[u] = 2
        undecided = [v for v in undecided if state[v] == 0]
    return [v for v in range(n) if state[v] == 1], count


def aggregates(adj, seed, roots):
    """(agg, vertices assigned in phase 2)"""
    n = len(adj)
    h = [CC.priority(v, seed) for v in range(n)]
    first = [-1] * n
    for k, r in enumerate(roots):
        first[r] = k
        for u in adj[r]:
            first[u] = k  # unique: two roots are never within distance 2
    agg = list(first)
    late = 0
    for v in range(n):
        if first[v] >= 0:
            continue
        best = -1
        for u in adj[v]:
            if first[u] >= 0 and (best < 0 or _precedes(h, u, best)):
                best = u
        assert best >= 0, "maximality: a vertex that is out has a phase-1 neighbour"
        agg[v] = first[best]
        late += 1
    return agg, late


class Aggregation(object):
    def __init__(self, S, seed):
        adj = CC.adjacency(S)
        self.n = len(adj)
        roots, self.rounds = round_roots(adj, seed)
        agg, self.phase2 = aggregates(adj, seed, roots)
        self.roots = np.array(roots, dtype=np.int32)
        self.agg = np.array(agg, dtype=np.int32)
        self.count = len(roots)
        sizes = np.bincount(self.agg, minlength=self.count) if self.n else np.zeros(0, dtype=np.int64)
        self.largest = int(sizes.max()) if self.n else 0
        self.smallest = int(sizes.min()) if self.n else 0
        self.max_degree = max((len(a) for a in adj), default=0)
        for a in (self.roots, self.agg):
            a.setflags(write=False)

    def info(self):
        """info[0..5] and info[7] of spl_matrix_aggregate"""
        return [self.n, self.count, self.rounds, self.largest, self.smallest, self.max_degree, self.phase2]


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    """the yardstick's aggregation of a committed pattern of tests/coloring_cases.py; computed once, read-only"""
    return Aggregation(CC.pattern(name), seed)


# ---- the hierarchy by scipy --------------------------------------------------------------------------------------------
def reciprocal(d):
    """1 / d_i: the IEEE quotient, Data.Complex's scaled one on complex values; a zero gives inf / NaN, never an error"""
    with np.errstate(all="ignore"):
        if np.iscomplexobj(d):
            q = [TK.c_div(1.0, 0.0, re, im) for re, im in zip(d.real.tolist(), d.imag.tolist())]
            return K._cvec([p[0] for p in q], [p[1] for p in q])
        return np.array([TK.ieee_div(1.0, v) for v in d.tolist()], dtype=np.float64)


def omega_of(nrm):
    return 4.0 / (3.0 * nrm)  # two rounded operations


def weights(omega, dinv):
    """w = omega * dinv: (omega :+ 0) times dinv by Data.Complex's product on complex values"""
    with np.errstate(all="ignore"):
        if np.iscomplexobj(dinv):
            return K.Complex.scaled((omega, 0.0), dinv)
        return omega * dinv


def tentative(agg, count, dtype):
    n = len(agg)
    return sp.csr_matrix((np.ones(n, dtype=dtype), np.asarray(agg, dtype=np.int64), np.arange(n + 1)), shape=(n, count))


class Level(object):
    """A, P, R as scipy CSR with sorted indices (P and R None on the coarsest level), and w"""

    def __init__(self, A, w, P=None, R=None):
        self.A, self.w, self.P, self.R = A, w, P, R
        self.n = A.shape[0]


def _product(X, Y):
    """X Y by scipy with sorted rows in and out: every entry is then summed over ascending k, as the header has it"""
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    X.sort_indices()
    Y.sort_indices()
    Z = sp.csr_matrix(X @ Y)
    Z.sort_indices()
    return Z


def scipy_hierarchy(S, seed=0, coarse_size=256, max_levels=16, plain=False):
    """the level recurrence of the header with scipy's own products: the same matrices up to rounding"""
    A = sp.csr_matrix(S)
    A.sort_indices()
    levels = []
    while True:
        n = A.shape[0]
        d = A.diagonal()
        dinv = reciprocal(d)
        with np.errstate(all="ignore"):
            scaled = sp.diags(dinv) @ A if n else A
            nrm = float(abs(scaled).sum(axis=1).max()) if n and A.nnz else 0.0
            w = weights(omega_of(nrm), dinv)
        if n <= coarse_size or len(levels) + 1 == max_levels:
            levels.append(Level(A, w))
            return levels
        g = Aggregation(A, seed)
        if g.count == n:
            levels.append(Level(A, w))
            return levels
        T = tentative(g.agg, g.count, A.dtype)
        if plain:
            P = T
        else:
            # diag(w) A on A's own sorted pattern: scipy's product leaves its rows unsorted, and the next product would
            # then add its terms in another order than the header's ascending one
            rows = np.repeat(np.arange(n), np.diff(A.indptr))
            with np.errstate(all="ignore"):
                WA = sp.csr_matrix((K.arithmetic(np.iscomplexobj(w)).entrywise(w[rows], A.data), A.indices, A.indptr),
                                   shape=A.shape)
                P = sp.csr_matrix(T - _product(WA, T))
        P.sort_indices()
        R = sp.csr_matrix(P.conj().T)
        R.sort_indices()
        levels.append(Level(A, w, P, R))
        with np.errstate(all="ignore"):
            A = _product(R, _product(A, P))


def operator_complexity(levels):
    return sum(L.A.nnz for L in levels) / float(levels[0].A.nnz)


# ---- the cycle ---------------------------------------------------------------------------------------------------------
def _accumulated(op, x, y):
    """y + op x with every row's sum continued from y_r in ascending column order (the product with `accumulate`)"""
    y = y.copy()
    for rows, vals, cols in op.steps:
        y[rows] = y[rows] + op.A.entrywise(vals, x[cols])
    return y


class Cycle(object):
    """x = cycle(0, b) of the header on the given levels: a fixed linear operator, the M of krylov_cases.cg / bicgstab"""
    none = False

    def __init__(self, levels, sweeps=1, coarse_sweeps=4):
        self.nu, self.coarse = sweeps, coarse_sweeps
        self.ops = []
        for L in levels:
            self.ops.append((K.RowSerial(L.A), None if L.P is None else K.RowSerial(L.P),
                             None if L.R is None else K.RowSerial(L.R), L.w))
        self.arith = K.arithmetic(np.iscomplexobj(levels[0].w))

    def _sweep(self, l, x, b):
        A, _, _, w = self.ops[l]
        return x + self.arith.entrywise(w, b - A(x))

    def _cycle(self, l, b):
        A, P, R, w = self.ops[l]
        x = self.arith.entrywise(w, b)  # the first sweep from x = 0
        if l == len(self.ops) - 1:
            for _ in range(self.coarse - 1):
                x = self._sweep(l, x, b)
            return x
        for _ in range(self.nu - 1):
            x = self._sweep(l, x, b)
        r = b - A(x)
        e = self._cycle(l + 1, R(r))
        x = _accumulated(P, e, x)
        for _ in range(self.nu):
            x = self._sweep(l, x, b)
        return x

    def __call__(self, b):
        with np.errstate(all="ignore"):
            return self._cycle(0, np.asarray(b, dtype=self.arith.dtype))


@functools.lru_cache(maxsize=None)
def cached_hierarchy(name, coarse_size=256, plain=False):
    return tuple(scipy_hierarchy(K.matrix(name), 0, coarse_size, 16, plain))


@functools.lru_cache(maxsize=None)
def solve_reference(method, name, coarse_size=256):
    """the restated driver of tests/krylov_cases.py with the restated cycle on the scipy hierarchy (defaults)"""
    M = Cycle(cached_hierarchy(name, coarse_size), DEFAULTS["sweeps"], DEFAULTS["coarse_sweeps"])
    out = K.DRIVERS[method](K._operator(name), K.rhs(name), M, None, K.RTOL, 0.0, 2000)
    out.x.setflags(write=False)
    out.history.setflags(write=False)
    return out


def poisson3d(m):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    S = sp.csr_matrix(sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T))
    S.sort_indices()
    return S


if __name__ == "__main__":  # what every committed case does: checked here, without a GPU
    for name in CC.NAMES:
        for seed in SEEDS:
            g = reference(name, seed)
            print("%-12s seed %d  n %5d  aggregates %5d  rounds %3d  sizes %3d .. %3d  degree %4d  phase 2 %5d"
                  % (name, seed, g.n, g.count, g.rounds, g.smallest, g.largest, g.max_degree, g.phase2))
    for method, name in K.CASES:
        for coarse in (256, 16):
            levels = cached_hierarchy(name, coarse)
            out = solve_reference(method, name, coarse)
            none = K.reference(method, name, None)
            print("%-8s %-9s coarse_size %3d levels %-22s complexity %.2f  iterations %4d -> %3d  reason %s  residual %.2e"
                  % (method, name, coarse, " / ".join(str(L.n) for L in levels), operator_complexity(levels),
                     none.iterations, out.iterations, K.REASONS[out.reason],
                     K.true_relative_residual(K.matrix(name), out.x, K.rhs(name))))
    print("poisson3d(16): levels %s" % " / ".join(str(L.n) for L in scipy_hierarchy(poisson3d(16))))
