"""Inputs and the yardstick of tests/test_gpu_coloring.py and tests/test_coloring_cpu.py.

The yardstick restates the section "multicolour ordering on handles" of include/sparse_linear_hip.h in Python integers:

  * the priority h(v): the splitmix64 finaliser of v + 0x9E3779B97F4A7C15 (seed + 1) mod 2^64; u precedes v when
    h(u) > h(v), or they are equal and u < v;
  * the graph: {i, j}, i != j, is an edge when (i, j) or (j, i) is STORED, explicit zeros included;
  * the colouring, twice: `greedy` walks the vertices in priority order and gives each the smallest colour none of its
    (already coloured, hence preceding) neighbours has, with round(v) = 1 + max round over them; `rounds` simulates the
    launches, where every uncoloured vertex whose preceding neighbours all carried a colour when the round began takes
    its colour.  The two must agree (tests/test_coloring_cpu.py), and the device must give both (the GPU test);
  * the permutation: the vertices by colour, then by ascending index; the offsets: the class boundaries in it.

`python tests/coloring_cases.py` prints what every committed pattern does, without a GPU."""
import functools

import numpy as np
import scipy.sparse as sp

import krylov_cases as K

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SEEDS = (0, 7)


def priority(v, seed):
    z = (v + GOLDEN * (seed + 1)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def adjacency(S):
    """the neighbours of every vertex as sorted lists: the stored positions of S and of its transpose, the diagonal
    left out; values are not looked at (an explicit zero is an entry)"""
    S = sp.csr_matrix(S)
    n = S.shape[0]
    rows = np.repeat(np.arange(n), np.diff(S.indptr))
    cols = S.indices
    keep = rows != cols
    r, c = np.concatenate([rows[keep], cols[keep]]), np.concatenate([cols[keep], rows[keep]])
    P = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))  # duplicates are summed: one entry per edge and side
    P.sort_indices()
    ptr, idx = P.indptr.tolist(), P.indices.tolist()
    return [idx[ptr[v]:ptr[v + 1]] for v in range(n)]


def _order(n, seed):
    h = [priority(v, seed) for v in range(n)]
    return h, sorted(range(n), key=lambda v: (-h[v], v))


def greedy(adj, seed):
    """(colours, rounds of every vertex) of the serial first-fit colouring in priority order"""
    n = len(adj)
    _, order = _order(n, seed)
    colour, rnd = [-1] * n, [0] * n
    for v in order:
        taken = set()
        r = 0
        for u in adj[v]:
            if colour[u] >= 0:  # coloured before v: u precedes v
                taken.add(colour[u])
                r = max(r, rnd[u])
        c = 0
        while c in taken:
            c += 1
        colour[v], rnd[v] = c, r + 1
    return colour, rnd


def rounds(adj, seed):
    """(colours, number of rounds) of the simulated launches"""
    n = len(adj)
    h, _ = _order(n, seed)
    before = [[u for u in adj[v] if h[u] > h[v] or (h[u] == h[v] and u < v)] for v in range(n)]
    colour = [-1] * n
    work = list(range(n))
    count = 0
    while work:
        count += 1
        ready = [v for v in work if all(colour[u] >= 0 for u in before[v])]  # decided on the state of the round's start
        fresh = {}
        for v in ready:
            taken = {colour[u] for u in before[v]}
            c = 0
            while c in taken:
                c += 1
            fresh[v] = c
        for v, c in fresh.items():
            colour[v] = c
        work = [v for v in work if v not in fresh]
    return colour, count


def classes(colour):
    """(perm, offsets): the vertices by colour and then by ascending index, and the class boundaries"""
    colour = np.asarray(colour, dtype=np.int64)
    perm = np.argsort(colour, kind="stable").astype(np.int32)
    ncolors = int(colour.max()) + 1 if len(colour) else 0
    offsets = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=ncolors))]).astype(np.int64)
    return perm, offsets


def number_of_levels(S, lower):
    """the levels of the triangular solve with the strict lower (or upper) part of S's pattern: 0 for an empty matrix"""
    S = sp.csr_matrix(S)
    n = S.shape[0]
    ptr, idx = S.indptr.tolist(), S.indices.tolist()
    level = [0] * n
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        deps = [level[k] + 1 for k in idx[ptr[i]:ptr[i + 1]] if (k < i if lower else k > i)]
        level[i] = max(deps) if deps else 1
    return max(level) if n else 0


def permuted(S, perm):
    S = sp.csr_matrix(S)[perm][:, perm]
    S.sort_indices()
    return S


# ---- the committed patterns --------------------------------------------------------------------------------------------
NAMES = ("poisson", "unsym", "upper", "chain", "dense_chain", "star", "diagonal", "one", "empty", "zeros", "hermitian")


def _chain(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n), format="csr")


@functools.lru_cache(maxsize=None)
def pattern(name):
    """scipy CSR with sorted indices.
    poisson:     the 91 x 91 five-point Laplacian of tests/krylov_cases.py
    unsym:       its n = 300 unsymmetric matrix: most edges are stored on one side only
    upper:       n = 200, strictly upper triangular, about six entries a row: EVERY edge is stored on one side only and
                 no diagonal is stored
    chain:       tridiagonal, 5000 rows
    dense_chain: blockdiag(dense 70 x 70, chain of 200): 70 colours (the second window of 64) and 70 rounds
    star:        n = 1000, row 0 and column 0 full, the diagonal
    diagonal:    n = 50, no edge
    one, empty:  n = 1, n = 0
    zeros:       n = 150: a diagonal of ones and explicit ZEROS above it, which are edges all the same
    hermitian:   the complex Hermitian matrix on poisson's pattern"""
    if name in ("poisson", "unsym", "hermitian"):
        return K.matrix(name)
    if name == "upper":
        rng = np.random.default_rng(2101)
        n = 200
        r = np.repeat(np.arange(n - 1), 6)
        c = rng.integers(r + 1, n)
        S = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
        S.data[:] = 1.0
    elif name == "chain":
        S = _chain(5000)
    elif name == "dense_chain":
        S = sp.csr_matrix(sp.block_diag([np.ones((70, 70)), _chain(200)]))
    elif name == "star":
        n = 1000
        first = np.zeros(n - 1, dtype=np.int64)
        rest = np.arange(1, n)
        r = np.concatenate([first, rest, np.arange(n)])
        c = np.concatenate([rest, first, np.arange(n)])
        S = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    elif name == "diagonal":
        S = sp.identity(50, format="csr")
    elif name == "one":
        S = sp.csr_matrix(np.array([[3.0]]))
    elif name == "empty":
        S = sp.csr_matrix((0, 0))
    elif name == "zeros":
        rng = np.random.default_rng(2102)
        n = 150
        r = np.repeat(np.arange(n - 1), 3)
        c = rng.integers(r + 1, n)
        pairs = np.unique(np.stack([r, c], axis=1), axis=0)
        rr, cc = np.concatenate([pairs[:, 0], np.arange(n)]), np.concatenate([pairs[:, 1], np.arange(n)])
        vv = np.concatenate([np.zeros(len(pairs)), np.ones(n)])
        S = sp.csr_matrix((vv, (rr, cc)), shape=(n, n))  # the zeros stay entries
        assert S.nnz == len(pairs) + n
    else:
        raise KeyError(name)
    S = sp.csr_matrix(S)
    S.sort_indices()
    return S


class Reference(object):
    def __init__(self, name, seed):
        adj = adjacency(pattern(name))
        self.n = len(adj)
        colour, rnd = greedy(adj, seed)
        self.colors = np.array(colour, dtype=np.int32)
        self.rounds = max(rnd) if rnd else 0
        self.ncolors = int(self.colors.max()) + 1 if self.n else 0
        self.perm, self.offsets = classes(colour)
        self.max_degree = max((len(a) for a in adj), default=0)
        for a in (self.colors, self.perm, self.offsets):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    """the yardstick's colours, rounds, permutation and offsets of a committed pattern; computed once, read-only"""
    return Reference(name, seed)


# ---- the solves in the new numbering -----------------------------------------------------------------------------------
SOLVES = (("cg", "poisson"), ("cg", "hermitian"), ("bicgstab", "unsymz"))


def solve_reference(method, name, kind, mid=None, seed=0):
    """the restated driver of tests/krylov_cases.py on S[perm][:, perm] with b[perm], its x scattered back to the
    original numbering: (x, Outcome).  `unsymz` has the pattern of its own matrix; mid: the middle part the device was
    given, where the test did not make it by the yardstick's own quotient"""
    S, b = K.matrix(name), np.array(K.rhs(name))
    colour, _ = greedy(adjacency(S), seed)
    perm, _ = classes(colour)
    Sp = permuted(S, perm)
    out = K.DRIVERS[method](Sp, b[perm], K.preconditioner(Sp, kind, mid), None, K.RTOL, 0.0, 2000)
    x = np.empty_like(out.x)
    x[perm] = out.x
    return x, out


@functools.lru_cache(maxsize=None)
def cached_solve_reference(method, name, kind):
    x, out = solve_reference(method, name, kind)
    x.setflags(write=False)
    out.history.setflags(write=False)
    return x, out


if __name__ == "__main__":  # what every committed pattern does: checked here, without a GPU
    for name in NAMES:
        for seed in SEEDS:
            ref = reference(name, seed)
            S = permuted(pattern(name), ref.perm) if ref.n else pattern(name)
            print("%-12s seed %d  n %5d  colours %3d  rounds %3d  classes %s  degree %4d  levels %5d -> %3d / %3d"
                  % (name, seed, ref.n, ref.ncolors, ref.rounds, np.diff(ref.offsets).tolist()[:6], ref.max_degree,
                     number_of_levels(pattern(name), True), number_of_levels(S, True), number_of_levels(S, False)))
