"""Signed, wide-range and non-finite data for the SpMV kernels, with an exact reference.  Pure numpy / Python: no GPU,
no oracle.

Two small matrices, built from a fixed seed (pattern(name)):

  edge   1127 x 1500, rectangular, ncols no multiple of 2^4 or 2^9.  Ordinary rows hold 0 ... 24 entries, every 7th row
         is empty, row 449 holds 700 entries (longer than the CSR-stream kernel's 512-entry chunk and than a 64-entry
         unit), the hub column 777 is stored by 190 rows, three rows hold nothing but the last column, and the panel of
         rows 192 ... 255 has, at P = 64, w = 4, an index block (columns 80 ... 95) with exactly 64 entries, one (160 ...
         175) with exactly 128 and two (240 ... 255, 256 ... 271) with none; every other segment is ragged.  The hub has
         190 rows and not 300: every row that stores a poisoned column is non-finite, and at least 3/4 of the rows must
         stay finite under `poison`.
  band   1000 x 1000, the 9 diagonals -4 ... 4, boundary rows shortened: 36 padded entries of 9000 in a sliced-ELL
         image, so the image contains padding and stays under 1/8 of nnz.

Value sets (case(matrix, values)): signed, wide, tiny, huge, poison, and the complex signed_z, poison_z.  poison shares
its matrix values with signed (stored 0.0 and -0.0 in poisoned columns included), so one device handle serves both and
the `signed` run is the poison run "with the poison replaced by finite values".

exact_rows() gives the exact row sums (fractions.Fraction), sum |a x| (+ |y0|) per row and the class of every row:
finite, +inf, -inf or NaN.  The class is derived from the separately rounded products a * x and y0 alone: NaN if one of
them is NaN or both infinities occur, else the infinity that occurs, else finite.  An overflowing product (huge) counts
as the infinity it rounds to.  For these inputs the class does not depend on the summation order: no finite partial sum
can overflow.  A complex row is two real rows of 2 len terms: re = sum ar xr + (-ai) xi, im = sum ar xi + ai xr.

check() holds a result against that: finite rows within gamma_n sum |a x| (any summation order of separately rounded
products satisfies it), the other rows by class, and in reference mode every non-NaN value bit for bit against the
oracle's result."""
import functools
from fractions import Fraction

import numpy as np

SEED = 20260

U = Fraction(1, 2 ** 53)
TINY_ABS = Fraction(1, 2 ** 1074)     # the smallest subnormal: the absolute error of one underflowing product is half of it
FINITE, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+inf", "-inf", "NaN")

REAL_SETS = ("signed", "wide", "tiny", "huge", "poison")
COMPLEX_SETS = ("signed_z", "poison_z")
STREAM_CHUNK = 512                    # rows longer than this: the documented wavefront tree of the CSR-stream kernels

HUB = 777
LONG_ROW = 449
EXACT_PANEL = 3                       # rows 192 ... 255
ORDINARY = (333, 1234)                # two ordinary poisoned columns


class Pattern(object):
    """CSR pattern, column indices ascending inside a row"""

    def __init__(self, name, nrows, ncols, rows, cols):
        key = np.unique(rows.astype(np.int64) * ncols + cols.astype(np.int64))
        self.name, self.nrows, self.ncols = name, nrows, ncols
        self.rows, self.cols = key // ncols, key % ncols
        self.rowptr = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=nrows))]).astype(np.int64)
        self.lens = np.diff(self.rowptr)
        self.nnz = len(key)

    def row(self, r):
        return slice(int(self.rowptr[r]), int(self.rowptr[r + 1]))


def _edge():
    rng = np.random.default_rng(SEED)
    nr, nc = 1127, 1500
    lens = rng.integers(0, 25, nr)
    lens[::7] = 0
    lens[LONG_ROW] = 0
    rows = np.repeat(np.arange(nr), lens)
    cols = rng.integers(0, nc, len(rows))
    # the panel with engineered segments: clear its four index blocks, then fill two of them
    lo, hi = 64 * EXACT_PANEL, 64 * EXACT_PANEL + 64
    blk = cols >> 4
    keep = ~((rows >= lo) & (rows < hi) & np.isin(blk, (5, 10, 15, 16)))
    rows, cols = rows[keep], cols[keep]
    live = np.array([r for r in range(lo, hi) if r % 7])
    extra_r, extra_c = [], []
    for b, count in ((5, 64), (10, 128)):
        cells = rng.choice(len(live) * 16, count, replace=False)
        extra_r.append(live[cells // 16])
        extra_c.append(16 * b + cells % 16)
    # one long row, one hub column, rows that hold only the last column, more rows in the first column of an index block
    extra_r.append(np.full(700, LONG_ROW))
    extra_c.append(rng.choice(nc, 700, replace=False))
    others = np.array([r for r in range(nr) if r % 7 and not lo <= r < hi and r != LONG_ROW])
    extra_r.append(rng.choice(others, 190, replace=False))
    extra_c.append(np.full(190, HUB))
    last_only = np.array([14, 700, 1120])                    # multiples of 7: empty so far
    extra_r.append(last_only)
    extra_c.append(np.full(3, nc - 1))
    for c in (0, 16, 512):
        extra_r.append(rng.choice(others, 10, replace=False))
        extra_c.append(np.full(10, c))
    extra_r.append(np.array([100, 100]))                     # one row with a +inf and a -inf column under poison
    extra_c.append(np.array([0, 16]))
    P = Pattern("edge", nr, nc, np.concatenate([rows] + extra_r), np.concatenate([cols] + extra_c))
    # what the tests rely on
    assert np.all(P.lens[[r for r in range(0, nr, 7) if r not in last_only]] == 0)
    assert P.lens[LONG_ROW] == 700 and np.sum(P.cols == HUB) >= 190 and 12000 <= P.nnz <= 16000
    assert all(P.lens[r] == 1 and P.cols[P.row(r)][0] == nc - 1 for r in last_only)
    seg = np.bincount((P.cols >> 4)[(P.rows >= lo) & (P.rows < hi)], minlength=94)
    assert seg[5] == 64 and seg[10] == 128 and seg[15] == 0 and seg[16] == 0 and np.sum((seg > 0) & (seg % 64 != 0)) > 50
    return P


def _band():
    n = 1000
    r = np.repeat(np.arange(n), 9)
    c = r + np.tile(np.arange(-4, 5), n)
    ok = (c >= 0) & (c < n)
    P = Pattern("band", n, n, r[ok], c[ok])
    widths = np.array([P.lens[s:s + 64].max() for s in range(0, n, 64)])
    heights = np.array([len(P.lens[s:s + 64]) for s in range(0, n, 64)])
    pad = int(np.sum(widths * 64) - P.nnz)                   # slots of a SELL-64 image that hold no entry
    assert 0 < pad * 8 < P.nnz and np.sum(widths * heights) > P.nnz
    return P


@functools.lru_cache(maxsize=None)
def pattern(name):
    return {"edge": _edge, "band": _band}[name]()


def poisoned_columns(P):
    """column -> the value x takes there under poison"""
    inf, nan = float("inf"), float("nan")
    if P.name == "edge":
        return {0: inf, 16: -inf, 512: nan, P.ncols - 1: inf, HUB: inf, ORDINARY[0]: -inf, ORDINARY[1]: nan}
    # 9 rows per column in the band: more columns, so that every class still has its 20 rows
    return {0: inf, 16: -inf, 512: nan, P.ncols - 1: inf, 500: inf, 333: -inf, 901: nan, 100: inf, 200: inf, 600: -inf,
            604: inf, 700: -inf, 800: nan}   # rows 600 ... 604 store a +inf and a -inf column


class Case(object):
    """one (matrix, value set): CSR values, x, y0 for the accumulate form; complex arrays for the _z sets"""

    def __init__(self, P, name, vals, x, y0, clean=None):
        self.P, self.name, self.vals, self.x, self.y0, self.clean = P, name, vals, x, y0, clean
        self.is_complex = np.iscomplexobj(vals)
        for a in (vals, x, y0):
            a.setflags(write=False)

    def csc(self):
        """(nrows, ncols, colptr, rowidx, values): the tuple of the oracle and of the package's Matrix"""
        P = self.P
        order = np.argsort(P.cols, kind="stable")
        cp = np.concatenate([[0], np.cumsum(np.bincount(P.cols, minlength=P.ncols))]).astype(np.int64)
        return (P.nrows, P.ncols, cp, P.rows[order].astype(np.int64), self.vals[order])

    def csc_of_transpose(self):
        """the CSC tuple of A^T: A's CSR arrays as they stand (mulVT of this is A x)"""
        P = self.P
        return (P.ncols, P.nrows, P.rowptr.copy(), P.cols.astype(np.int64), self.vals.copy())

    def touched_rows(self):
        """rows that store a column where x differs from the clean case's, or whose y0 differs"""
        if self.clean is None:
            return np.zeros(self.P.nrows, dtype=bool)
        P = self.P
        t = np.zeros(P.nrows, dtype=bool)
        bad = np.array(sorted(poisoned_columns(P)))
        t[P.rows[np.isin(P.cols, bad)]] = True
        return t

    def touched_y0(self):
        if self.clean is None:
            return np.zeros(self.P.nrows, dtype=bool)
        a, b = _components(self.y0), _components(self.clean.y0)
        d = a.view(np.int64) != b.view(np.int64)
        return d.reshape(self.P.nrows, -1).any(axis=1)


def _components(a):
    return np.ascontiguousarray(a).view(np.float64) if np.iscomplexobj(a) else np.ascontiguousarray(a, dtype=np.float64)


def _cancel_rows(P):
    """a third of the rows with at least two entries: the ones whose entries are engineered to cancel"""
    r = np.arange(P.nrows)
    return (r % 3 == 1) & (P.lens >= 2) & (r != LONG_ROW)


def _zero_entries(P):
    """entries in poisoned columns that hold a stored 0.0 / -0.0: in rows that do not cancel"""
    cancel = _cancel_rows(P)
    bad = np.array(sorted(poisoned_columns(P)))
    k = np.nonzero(np.isin(P.cols, bad) & ~cancel[P.rows])[0]
    k = k[::3]                                       # every third of them
    return k[::2], k[1::2]                           # +0.0, -0.0


def _cancelling(P, vals, x):
    """consecutive pairs a x, -a x (1 + 2^-30) in the cancelling rows (the last group of an odd row is a triple closed
    by its last entry): sum |a x| >> |sum a x|"""
    vals = vals.copy()
    for r in np.nonzero(_cancel_rows(P))[0]:
        s = P.row(r)
        n = s.stop - s.start
        k = s.start
        while k < s.stop:
            g = 3 if s.stop - k == 3 else 2
            part = sum(float(vals[j]) * float(x[P.cols[j]]) for j in range(k, k + g - 1))
            xl = float(x[P.cols[k + g - 1]])
            vals[k + g - 1] = -part * (1.0 + 2.0 ** -30) / xl
            k += g
        assert n >= 2
    return vals


def _y0(rng, P, draw):
    y0 = draw(P.nrows)
    empty = np.nonzero(P.lens == 0)[0]
    y0[empty[::3]] = -0.0                            # must come back as -0.0 in the reference order
    return y0


def _signed(P, rng, x=None):
    x = rng.normal(size=P.ncols) if x is None else x
    vals = _cancelling(P, rng.normal(size=P.nnz), x)
    zp, zn = _zero_entries(P)
    vals[zp], vals[zn] = 0.0, -0.0
    return vals, x, _y0(rng, P, lambda n: rng.normal(size=n))


def _pow2(rng, n, lo, hi):
    m = rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    return np.ldexp(m, rng.integers(lo, hi + 1, n))


def _build(matrix, name):
    P = pattern(matrix)
    rng = np.random.default_rng([SEED, sum(map(ord, matrix + name))])
    if name == "signed":
        return Case(P, name, *_signed(P, rng))
    if name == "wide":            # |a x| <= 2^402, a row sum below 2^412: nothing over- or underflows
        return Case(P, name, _pow2(rng, P.nnz, -200, 200), _pow2(rng, P.ncols, -200, 200),
                    _y0(rng, P, lambda n: _pow2(rng, n, -200, 200)))
    if name == "tiny":            # every product is about 2^-1040: subnormal, 34 bits or fewer
        return Case(P, name, _pow2(rng, P.nnz, -520, -520), _pow2(rng, P.ncols, -520, -520),
                    _y0(rng, P, lambda n: _pow2(rng, n, -1040, -1040)))
    if name == "huge":
        x = rng.normal(size=P.ncols)
        big_cols = np.array([40, 641, 1000 if P.ncols > 1001 else 700, 975])
        x[big_cols] = [1e200, -1e200, 1e200, 1e200]
        vals, x, y0 = _signed(P, rng, x)
        k = np.nonzero(np.isin(P.cols, big_cols) & ~_cancel_rows(P)[P.rows] & (P.rows != LONG_ROW))[0][:12]
        assert len(k) >= 6
        vals[k] = np.where(np.arange(len(k)) % 2 == 0, 1e200, -1e200)   # a x = +-1e400: overflows
        return Case(P, name, vals, x, y0)
    if name == "poison":
        clean = case(matrix, "signed")
        x, y0 = clean.x.copy(), clean.y0.copy()
        for c, v in poisoned_columns(P).items():
            x[c] = v
        free = np.nonzero(~Case(P, name, clean.vals.copy(), x.copy(), y0.copy(), clean).touched_rows() & (P.lens > 0))[0]
        y0[free[5:11]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
        return Case(P, name, clean.vals.copy(), x, y0, clean)
    if name == "signed_z":
        re, im = case(matrix, "signed"), _signed(P, rng)
        return Case(P, name, re.vals + 1j * im[0], re.x + 1j * im[1], re.y0 + 1j * im[2])
    if name == "poison_z":        # poison in the real part, the imaginary part, or both
        clean = case(matrix, "signed_z")
        x, y0 = clean.x.copy(), clean.y0.copy()
        for i, (c, v) in enumerate(sorted(poisoned_columns(P).items())):
            x[c] = (complex(v, x[c].imag), complex(x[c].real, v), complex(v, v))[i % 3]
        free = np.nonzero(~Case(P, name, clean.vals.copy(), x.copy(), y0.copy(), clean).touched_rows() & (P.lens > 0))[0]
        y0[free[5:8]] = [complex(np.nan, 1.0), complex(2.0, np.inf), complex(-np.inf, np.nan)]
        return Case(P, name, clean.vals.copy(), x, y0, clean)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(matrix, name):
    c = _build(matrix, name)
    _self_check(c)
    return c


# ---- the exact reference ----------------------------------------------------------------------------------------
def _terms(c):
    """per virtual row (a real row, or one component of a complex row): the factor arrays (a, x), the number of terms
    per stored entry, y0 per virtual row, the virtual row of every term"""
    P = c.P
    if not c.is_complex:
        return c.vals, c.x[P.cols], 1, np.asarray(c.y0), P.rows
    ar, ai = c.vals.real, c.vals.imag
    xr, xi = c.x.real[P.cols], c.x.imag[P.cols]
    # entry k gives the terms (ar xr, -ai xi) of row 2r and (ar xi, ai xr) of row 2r + 1
    a = np.stack([ar, -ai, ar, ai], axis=1).ravel()
    x = np.stack([xr, xi, xi, xr], axis=1).ravel()
    rows = np.stack([2 * P.rows, 2 * P.rows, 2 * P.rows + 1, 2 * P.rows + 1], axis=1).ravel()
    return a, x, 2, _components(c.y0), rows


class Exact(object):
    """what exact_rows returns, per virtual row i (a real row, or one component of a complex row; per of them to a
    row): cls[i], total[i] (Fraction; None on a non-finite row), sabs[i] (Fraction), lens[i] (stored entries), n[i]
    (the n of gamma_n)"""

    def __init__(self, per, cls, total, sabs, lens, n):
        self.per, self.cls, self.total, self.sabs, self.lens, self.n = per, cls, total, sabs, lens, n
        self.nvirt = len(cls)


def exact_rows(c, accumulate=False):
    """exact row sums of A x (+ y0) with fractions.Fraction, per-row sum |a x| (+ |y0|) and classes; complex data per
    component with sum (|ar xr| + |ai xi|)"""
    a, xs, per, y, rows = _terms(c)
    nvirt = c.P.nrows * per
    with np.errstate(all="ignore"):
        p = a * xs
    cnt = np.zeros((4, nvirt), dtype=np.int64)
    np.add.at(cnt, (classes(p), rows), 1)
    if accumulate:
        np.add.at(cnt, (classes(y), np.arange(nvirt)), 1)
    cls = np.where((cnt[NAN] > 0) | ((cnt[PINF] > 0) & (cnt[NINF] > 0)), NAN,
                   np.where(cnt[PINF] > 0, PINF, np.where(cnt[NINF] > 0, NINF, FINITE)))
    total = [Fraction(0)] * nvirt
    sabs = [Fraction(0)] * nvirt
    fin = cls == FINITE
    al, xl, rl = a.tolist(), xs.tolist(), rows.tolist()
    for k in range(len(al)):
        r = rl[k]
        if fin[r]:
            t = Fraction(al[k]) * Fraction(xl[k])
            total[r] += t
            sabs[r] += abs(t)
    if accumulate:
        yl = y.tolist()
        for r in range(nvirt):
            if fin[r]:
                total[r] += Fraction(yl[r])
                sabs[r] += abs(Fraction(yl[r]))
    lens = np.repeat(c.P.lens, per)
    n = (2 * lens + 1) if per == 2 else (lens + (1 if accumulate else 0))
    return Exact(per, cls, [t if f else None for t, f in zip(total, fin)], sabs, lens, n)


_exact_cached = functools.lru_cache(maxsize=None)(exact_rows)


def gamma(n):
    return n * U / (1 - n * U)


def classes(v):
    v = _components(v)
    return np.where(np.isnan(v), NAN, np.where(v == np.inf, PINF, np.where(v == -np.inf, NINF, FINITE)))


def _bits(v):
    return _components(v).view(np.int64)


def check(got, c, accumulate, mode, ref=None, clean_got=None, tree_over=None):
    """got: what a kernel (or the oracle) delivered for case c, y = A x or y <- A x + y0.  Raises AssertionError.

    mode "free": finite rows within gamma_n sum |a x| of the exact sum (+ len 2^-1074 for `tiny`; zeros compare with
    ==), the other rows by class.  mode "reference": the same, and every non-NaN value bit for bit equal to ref (the
    oracle's result), NaN where ref is NaN; rows longer than tree_over (the CSR-stream kernel's documented tree) are
    exempt from the bits, not from the bound.  clean_got: the same kernel's result on c.clean (poison replaced by
    finite values): rows that store no poisoned column and keep their y0 must equal it, bit for bit in reference mode,
    and are finite rows under the bound in free mode."""
    assert mode in ("free", "reference")
    e = _exact_cached(c, bool(accumulate))
    g = _components(got)
    assert g.shape == (e.nvirt,), "result of %s, expected %d values" % (g.shape, e.nvirt)
    gc = classes(g)
    wrong = np.nonzero(gc != e.cls)[0]
    assert len(wrong) == 0, "%s/%s: %d rows of the wrong class, first: row %d is %s, expected %s" % (
        c.P.name, c.name, len(wrong), wrong[0] // e.per, CLASS_NAMES[gc[wrong[0]]], CLASS_NAMES[e.cls[wrong[0]]])
    gl = g.tolist()
    absolute = TINY_ABS if c.name == "tiny" else 0
    for i in np.nonzero(e.cls == FINITE)[0]:
        bound = gamma(int(e.n[i])) * e.sabs[i] + int(e.lens[i]) * absolute
        err = abs(Fraction(gl[i]) - e.total[i])
        assert err <= bound, "%s/%s: row %d (%d entries) off by %.3e, bound %.3e, sum |a x| %.3e" % (
            c.P.name, c.name, i // e.per, e.lens[i], float(err), float(bound), float(e.sabs[i]))
    if mode == "reference":
        assert ref is not None
        r = _components(ref)
        compare = ~np.isnan(r)
        if tree_over is not None:
            compare &= e.lens <= tree_over
        d = np.nonzero(compare & (_bits(g) != _bits(r)))[0]
        assert len(d) == 0, "%s/%s: %d values differ from the reference's bits, first: row %d, %r against %r" % (
            c.P.name, c.name, len(d), d[0] // e.per, gl[d[0]], float(r[d[0]]))
    if clean_got is not None:
        assert c.clean is not None
        same = ~c.touched_rows()
        if accumulate:
            same &= ~c.touched_y0()
        same = np.repeat(same, e.per)
        assert np.all(e.cls[same] == FINITE)      # so the bound above has covered them in free mode
        if mode == "reference":
            if tree_over is not None:
                same &= e.lens <= tree_over
            d = np.nonzero(same & (_bits(g) != _bits(clean_got)))[0]
            assert len(d) == 0, "%s/%s: %d rows without a poisoned column differ from the unpoisoned run, first: row %d" % (
                c.P.name, c.name, len(d), d[0] // e.per)


# ---- the reference order in plain Python, and its mutants ----------------------------------------------------------
def _round(q):
    """a Fraction rounded once to double"""
    return float(q)   # int / int true division is correctly rounded


def fold(c, accumulate, skip_zeros=False, drop=None, fma=False, zero_start=False, flush_products=False):
    """the reference's y[r] = a * x + y[r] over the stored entries of a row in ascending column order, separately
    rounded (real cases), with one defect switched on at a time:
    skip_zeros: stored zeros are left out; drop: (row, position) of an entry that is left out; fma: a * x + y rounded
    once; zero_start: the accumulate form starts from 0.0 + y0; flush_products: subnormal products become 0"""
    assert not c.is_complex
    P = c.P
    v, x, cols = c.vals.tolist(), c.x.tolist(), P.cols.tolist()
    out = np.zeros(P.nrows)
    tiny = 2.0 ** -1022
    for r in range(P.nrows):
        acc = float(c.y0[r]) if accumulate else 0.0
        if zero_start:
            acc = 0.0 + acc
        s = P.row(r)
        for k in range(s.start, s.stop):
            a, xv = v[k], x[cols[k]]
            if (skip_zeros and a == 0.0) or (drop is not None and drop == (r, k - s.start)):
                continue
            if fma and all(map(np.isfinite, (a, xv, acc))):
                q = Fraction(a) * Fraction(xv) + Fraction(acc)
                acc = _round(q) if abs(q) < Fraction(2) ** 1024 else float("inf") * (1 if q > 0 else -1)
                continue
            p = a * xv
            if flush_products and abs(p) < tiny:
                p = 0.0
            acc = p + acc
        out[r] = acc
    return out


# ---- what every case must show, so that no test goes vacuous -----------------------------------------------------
def cancellation(c):
    """sum |a x| / |sum a x| per row (inf where the sum is 0), finite rows of y = A x"""
    e = _exact_cached(c, False)
    return np.array([float(s / abs(t)) if t else (np.inf if s else 1.0) for s, t in
                     ((e.sabs[i], e.total[i] if e.total[i] is not None else 0) for i in range(e.nvirt))])


def only_by_stored_zero(c):
    """rows of y = A x that are NaN under poison and would not be if stored zeros were skipped"""
    with_zeros = _exact_cached(c, False).cls
    kept = c.vals != 0
    P = c.P
    sub = Pattern(P.name, P.nrows, P.ncols, P.rows[kept], P.cols[kept])
    without = exact_rows(Case(sub, c.name, c.vals[kept].copy(), c.x.copy(), c.y0.copy())).cls
    return (with_zeros == NAN) & (without != NAN)


def _self_check(c):
    e = _exact_cached(c, False)
    ea = _exact_cached(c, True)
    if c.name in ("signed", "wide", "tiny", "signed_z"):
        assert np.all(e.cls == FINITE) and np.all(ea.cls == FINITE)
    if c.name == "signed":
        assert np.sum(cancellation(c) > 2.0 ** 20) >= 200
        assert np.sum(c.vals == 0) >= 10
    if c.name == "tiny":
        with np.errstate(all="ignore"):
            p = np.abs(c.vals * c.x[c.P.cols])
        assert np.all((p > 0) & (p < 2.0 ** -1022))
    if c.name == "huge":
        assert 4 <= np.sum(e.cls != FINITE) <= 40 and np.sum(e.cls == PINF) and np.sum(e.cls == NINF)
    if c.name.startswith("poison"):
        rows = c.P.nrows
        nonfinite = (ea.cls != FINITE).reshape(rows, -1).any(axis=1)
        assert 4 * np.sum(~nonfinite) >= 3 * rows, "only %d of %d rows stay finite" % (np.sum(~nonfinite), rows)
        for k in (NAN, PINF, NINF):
            assert np.sum((e.cls == k).reshape(rows, -1).any(axis=1)) >= 20, CLASS_NAMES[k]
        # y0 carries -0.0 on empty rows and each non-finite class on rows without a poisoned column
        y = _components(c.y0)
        assert np.sum(np.signbit(y) & (y == 0)) >= (10 if np.any(c.P.lens == 0) else 0) and np.sum(np.isnan(y)) and np.sum(y == np.inf) and np.sum(y == -np.inf)
        assert not np.any(c.touched_rows() & c.touched_y0())
    if c.name == "poison":
        assert np.sum(only_by_stored_zero(c)) >= 10
        x = c.x[c.P.cols]
        has_p = np.bincount(c.P.rows[x == np.inf], minlength=c.P.nrows) > 0
        has_n = np.bincount(c.P.rows[x == -np.inf], minlength=c.P.nrows) > 0
        assert np.any(has_p & has_n)
