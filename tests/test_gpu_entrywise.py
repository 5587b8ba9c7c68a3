"""The entry-wise layer on device handles: spl_matrix_map, _scale_rows_cols, _filter, _band, _reduce_dev, _norm and
their Python mirrors on DeviceMatrix.

Expected values come from numpy on the input arrays and from the restatements in this file (np_magnitude, np_map,
np_scale_rows_cols, np_filter, np_band), the exact sums from math.fsum; none from the library under test.  Doubles are
compared as uint64.  One exception is stated where it applies (same_values): where the restatement's ARITHMETIC yields
a NaN (inf - inf, inf / inf, a NaN operand), IEEE 754 leaves the NaN's sign and payload to the implementation, and the
device need only give a NaN there; NaNs that are moved or have their sign bit set, cleared or flipped are compared bit
for bit like everything else.

Base matrices, built the way tests/test_gpu_submatrix.py builds its own: a real 6 007 x 4 099 matrix with about 60 000
entries (mean row length 10), empty rows at both ends and in the middle, one row of 300 entries; values that are
rounding-sensitive doubles salted with -0.0, +0.0, +inf, -inf, a NaN with a payload, a subnormal, 1e300 and 1e-300; a
complex copy with its own imaginary parts; and narrow matrices with mean row lengths of about 1, 2, 3, 7, 25 and 100,
which together with the base make the host choose every group width G = 1, 2, 4 ... 64 in the count, write and
reduction passes.

Bounds.  abs-sums: for every slice |got - exact| <= (len + 4) 2^-53 sum|a|, exact = math.fsum of the moduli — any
order of len - 1 additions errs by at most (len - 1) u sum|a| to first order (u = 2^-53), the magnitude of a complex
entry by at most 2 u of itself (two squares, a sum, a square root; the scalings are exact), and the remaining 3 u cover
the second-order terms.  Frobenius norm: relative (nnz + 4) u."""
import collections
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NR, NC = 6007, 4099
EMPTY_ROWS = (0, 1, 2001, 2002, 2003, NR - 2, NR - 1)
LONG_ROW, LONG_LEN = 3000, 300
BLOCK = (2002, 4004)  # part 1 of 3 of the rows: holds empty rows and the long row
NAN_PAYLOAD = np.array([0x7FF80000DEADBEEF], dtype=np.uint64).view(np.float64)[0]
NAN_PAYLOAD_IM = np.array([0xFFF8000000C0FFEE], dtype=np.uint64).view(np.float64)[0]
SIGN = np.uint64(0x8000000000000000)
U = 2.0 ** -53
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

Csr = collections.namedtuple("Csr", "nrows ncols rp ci v")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def same_values(got, want):
    """bit for bit, except where `want` is a NaN that arithmetic made: a NaN is needed there, whichever"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    g, w = got.view(np.float64), want.view(np.float64)
    nan = np.isnan(w)
    odd = np.flatnonzero(~nan & (bits(g) != bits(w)))
    if len(odd) or not np.all(np.isnan(g[nan])):
        print("entries whose bits differ: %r; device %r, numpy %r" % (odd[:8].tolist(), bits(g)[odd[:8]].tolist(),
                                                                       bits(w)[odd[:8]].tolist()))
        return False
    return True


# ---- numpy on the input arrays: the expected values ----------------------------------------------------------------

def csr_from_keys(nrows, ncols, keys, v):
    keys = np.asarray(keys, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    rows = keys[order] // ncols
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))]).astype(np.int64)
    return Csr(nrows, ncols, rp, (keys[order] % ncols).astype(np.int32), np.ascontiguousarray(np.asarray(v)[order]))


def row_ids(t):
    return np.repeat(np.arange(t.nrows, dtype=np.int64), np.diff(t.rp))


def np_keep(t, keep):
    rp = np.concatenate([[0], np.cumsum(np.bincount(row_ids(t)[keep], minlength=t.nrows))]).astype(np.int64)
    return Csr(t.nrows, t.ncols, rp, t.ci[keep], np.ascontiguousarray(t.v[keep]))


def np_rows(t, r0, r1):
    a, b = int(t.rp[r0]), int(t.rp[r1])
    return Csr(r1 - r0, t.ncols, t.rp[r0:r1 + 1] - a, t.ci[a:b], np.ascontiguousarray(t.v[a:b]))


def np_transpose(t):
    rows = row_ids(t)
    order = np.lexsort((rows, t.ci))
    rp = np.concatenate([[0], np.cumsum(np.bincount(t.ci, minlength=t.ncols))]).astype(np.int64)
    return Csr(t.ncols, t.nrows, rp, rows[order].astype(np.int32), np.ascontiguousarray(t.v[order]))


def np_exponent(x):
    """`exponent` of RealFloat: frexp's exponent, and 0 for 0"""
    return np.where(x == 0, 0, np.frexp(x)[1]).astype(np.int32)


def np_magnitude(x, y):
    """GHC's `magnitude`; inf / NaN by the header's rule where a part is not finite"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    finite = np.isfinite(x) & np.isfinite(y)
    xf, yf = np.where(finite, x, 1.0), np.where(finite, y, 1.0)
    k = np.maximum(np_exponent(xf), np_exponent(yf))
    a, b = np.ldexp(xf, -k), np.ldexp(yf, -k)
    aa, bb = a * a, b * b
    r = np.ldexp(np.sqrt(aa + bb), k)
    return np.where(finite, r, np.where(np.isinf(x) | np.isinf(y), np.inf, np.nan))


def np_moduli(t):
    if t.v.dtype == np.complex128:
        return np_magnitude(t.v.real.copy(), t.v.imag.copy())
    return (bits(t.v) & ~SIGN).view(np.float64)


def pack(re, im):
    z = np.empty(len(re), dtype=np.complex128)
    z.real, z.imag = re, im
    return z


def flip(x):
    return (bits(x) ^ SIGN).view(np.float64)


def cmul(a, b, c, d):
    """(a :+ b) * (c :+ d) of Data.Complex, every operation rounded once"""
    ac, bd, ad, bc = a * c, b * d, a * d, b * c
    return ac - bd, ad + bc


def np_map(v, op, s=None):
    """the header's statement of every map, on real arrays"""
    with np.errstate(all="ignore"):
        if v.dtype != np.complex128:
            if op == "negate":
                return flip(v)
            if op == "abs":
                return (bits(v) & ~SIGN).view(np.float64)
            if op == "signum":
                return np.where(v > 0, 1.0, np.where(v < 0, -1.0, v))
            if op in ("conj", "real"):
                return v.copy()
            if op == "imag":
                return np.zeros(len(v))
            return v * float(s)
        re, im = v.real.copy(), v.imag.copy()
        if op == "negate":
            return pack(flip(re), flip(im))
        if op == "conj":
            return pack(re, flip(im))
        if op == "real":
            return re
        if op == "imag":
            return im
        if op == "scale":
            return pack(*cmul(re, im, complex(s).real, complex(s).imag))
        r = np_magnitude(re, im)
        if op == "abs":
            return pack(r, np.zeros(len(re)))
        zero = (re == 0) & (im == 0)
        rr = np.where(zero, 1.0, r)
        return pack(np.where(zero, 0.0, re / rr), np.where(zero, 0.0, im / rr))


def np_scale_rows_cols(t, r, c, row0=0):
    rows, cols = row_ids(t), t.ci.astype(np.int64)
    with np.errstate(all="ignore"):
        if t.v.dtype != np.complex128:
            v = t.v.copy()
            if r is not None:
                v = r[rows] * v
            if c is not None:
                v = v * c[cols]
            return v
        re, im = t.v.real.copy(), t.v.imag.copy()
        if r is not None:
            re, im = cmul(r.real[rows].copy(), r.imag[rows].copy(), re, im)
        if c is not None:
            re, im = cmul(re, im, c.real[cols].copy(), c.imag[cols].copy())
        return pack(re, im)


def np_band(t, lo, hi, row0=0):
    d = t.ci.astype(np.int64) - (row_ids(t) + row0)
    keep = np.ones(len(d), dtype=bool)
    if lo is not None:
        keep &= d >= max(lo, I64_MIN)
    if hi is not None:
        keep &= d <= min(hi, I64_MAX)
    return np_keep(t, keep)


# ---- the base matrices ----------------------------------------------------------------------------------------------

def make_base():
    rng = np.random.default_rng(20_26)
    keys = np.unique(rng.integers(0, NR, 60_500) * NC + rng.integers(0, NC, 60_500))
    keys = keys[~np.isin(keys // NC, EMPTY_ROWS + (LONG_ROW,))]
    keys = np.concatenate([keys, LONG_ROW * NC + rng.choice(NC, LONG_LEN, replace=False)])
    v = rng.standard_normal(len(keys)) * 10.0 ** rng.integers(-3, 4, len(keys))  # rounding-order sensitive
    t = csr_from_keys(NR, NC, keys, v)
    v = t.v.copy()
    # the salt: at most one value that is not finite per row, the first entries of rows spread over the matrix
    firsts = t.rp[:-1][np.diff(t.rp) > 0]
    for k, value in ((5, -0.0), (300, 0.0), (700, np.inf), (1100, 5e-324), (1500, -0.0), (1900, 1e300), (2500, -np.inf),
                     (2900, 0.0), (3300, 1e-300), (3500, NAN_PAYLOAD), (4200, -0.0), (4600, -1e300)):
        v[firsts[k]] = value
    v[t.rp[LONG_ROW] + 150] = -0.0
    v[t.rp[LONG_ROW] + 151] = 0.0
    return t._replace(v=v)


def make_complex(t):
    rng = np.random.default_rng(7)
    im = rng.standard_normal(len(t.v)) * 10.0 ** rng.integers(-3, 4, len(t.v))
    im[::977] = -0.0
    im[12345] = NAN_PAYLOAD_IM
    # the real parts that are +0.0 and -0.0: zeros of every sign pattern, and the smallest number that is none
    pz, nz = np.flatnonzero((t.v == 0) & ~np.signbit(t.v)), np.flatnonzero((t.v == 0) & np.signbit(t.v))
    im[pz[0]], im[pz[1]] = -0.0, 5e-324       # (0, -0) goes, (0, 5e-324) stays
    im[nz[0]], im[nz[1]], im[nz[2]] = -0.0, 0.0, 5e-324
    return t._replace(v=pack(t.v, im))


NARROW = {"mean1": (3001, 517, 0.9), "mean2": (1501, 517, 1.8), "mean3": (2003, 517, 3.2), "mean7": (1201, 701, 7.0),
          "mean25": (601, 701, 25.0), "mean100": (301, 1031, 100.0)}


def make_narrow(name):
    nrows, ncols, mean = NARROW[name]
    rng = np.random.default_rng(len(name) + nrows)
    k = int(nrows * mean)
    keys = np.unique(rng.integers(0, nrows, k + k // 8) * ncols + rng.integers(0, ncols, k + k // 8))
    keys = rng.permutation(keys)[:k]
    return csr_from_keys(nrows, ncols, keys, rng.standard_normal(k))


def narrow_complex(t):
    rng = np.random.default_rng(t.nrows)
    return t._replace(v=pack(t.v, rng.standard_normal(len(t.v)) * 10.0 ** rng.integers(-2, 3, len(t.v))))


@pytest.fixture(scope="module")
def base():
    t = make_base()
    out = {"real": t, "complex": make_complex(t)}
    out.update((name, make_narrow(name)) for name in NARROW)
    return out


def test_base_matrices_are_what_the_tests_assume(base):
    t = base["real"]
    lens = np.diff(t.rp)
    assert (t.nrows, t.ncols) == (NR, NC) and 55_000 < len(t.ci) < 65_000
    assert all(lens[r] == 0 for r in EMPTY_ROWS) and lens[LONG_ROW] == LONG_LEN == lens.max()
    inside = np.ones(len(t.ci), dtype=bool)
    inside[t.rp[:-1][lens > 0]] = False
    assert np.all(np.diff(t.ci.astype(np.int64))[inside[1:]] > 0)  # strictly ascending inside every row
    nonfinite = np.bincount(row_ids(t)[~np.isfinite(t.v)], minlength=NR)
    assert nonfinite.max() == 1 and nonfinite.sum() == 3 and np.isnan(t.v).sum() == 1
    assert np.sum(np.signbit(t.v) & (t.v == 0)) == 4 and np.sum(~np.signbit(t.v) & (t.v == 0)) == 3
    assert 5e-324 in t.v and 1e300 in t.v and 1e-300 in t.v and -1e300 in t.v
    assert BLOCK[0] <= LONG_ROW < BLOCK[1] and lens[BLOCK[0]] == 0
    z = base["complex"]
    assert z.v.dtype == np.complex128 and same_bits(z.v.real, t.v) and np.isnan(z.v.imag).sum() == 1
    both_zero = (z.v.real == 0) & (z.v.imag == 0)
    assert both_zero.sum() >= 3 and np.any((z.v.real == 0) & (z.v.imag == 5e-324))
    groups = {name: 1 << int(np.ceil(np.log2(max(len(m.ci) / m.nrows, 1.0)))) for name, m in base.items()}
    assert sorted(set(min(g, 64) for g in groups.values())) == [1, 2, 4, 8, 16, 32, 64], groups


# ---- handles in, arrays out -------------------------------------------------------------------------------------------

def handle(torch, pkg, t):
    """the handle of a Csr through the device-array import: values are moved as bits"""
    cplx = t.v.dtype == np.complex128
    rp = torch.from_numpy(np.ascontiguousarray(t.rp, dtype=np.int64)).cuda()
    ci = torch.from_numpy(np.ascontiguousarray(t.ci, dtype=np.int64)).cuda()
    v = torch.from_numpy(np.ascontiguousarray(t.v)).cuda()
    torch.cuda.synchronize()
    n = len(t.ci)
    return pkg.DeviceMatrix.from_csr_dev(t.nrows, t.ncols, rp.data_ptr(), ci.data_ptr() if n else 0,
                                         v.data_ptr() if n else 0, index_width=8, complex=cplx)


def block_handle(pkg, t, r0, r1):
    """rows [r0, r1) of a real Csr as a row block of the whole"""
    sub = np_rows(t, r0, r1)
    return pkg.DeviceMatrix.from_csr(t.nrows, t.ncols, sub.rp, sub.ci, sub.v, row0=r0), sub


@pytest.fixture(scope="module")
def handles(gpu, pkg, base):
    return {name: handle(gpu, pkg, t) for name, t in base.items()}


@pytest.fixture(scope="module")
def block(gpu, pkg, base):
    return block_handle(pkg, base["real"], *BLOCK)


def assert_is(H, t, values=same_bits, row0=0, nrows_global=None):
    """H holds exactly t: dimensions, block, pointers, indices and values"""
    inf = H.info()
    assert (inf["nrows_global"], inf["ncols"], inf["row0"], inf["nrows_local"], inf["nnz"]) == \
        (t.nrows if nrows_global is None else nrows_global, t.ncols, row0, t.nrows, len(t.ci))
    assert H.is_complex == (t.v.dtype == np.complex128)
    rp, ci, v = H.export_csr()
    assert np.array_equal(rp, t.rp) and np.array_equal(ci, t.ci)
    assert v.dtype == t.v.dtype and values(v, t.v)


# ---- 1. maps --------------------------------------------------------------------------------------------------------

MAPS = (("negate", None), ("abs", None), ("signum", None), ("conj", None), ("real", None), ("imag", None),
        ("scale", -2.5), ("scale", 1.0 / 3.0))
MOVED = ("negate", "conj", "real", "imag")  # bits moved, set, cleared or flipped: no arithmetic anywhere


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_maps_against_the_restatements(gpu, base, handles, kind):
    t, H = base[kind], handles[kind]
    before = H.export_csr()
    cases = MAPS + ((("scale", 0.75 - 1.25j), ("scale", 2j)) if kind == "complex" else ())
    for op, s in cases:
        want = np_map(t.v, op, s)
        got = H.map(op, s) if s is not None else getattr(H, op)()
        exact = op in MOVED or (kind == "real" and op in ("abs", "signum"))
        assert_is(got, t._replace(v=want), values=same_bits if exact else same_values)
        assert got.is_complex == (kind == "complex" and op not in ("real", "imag")), op
    assert_is(-H, t._replace(v=np_map(t.v, "negate")))
    assert_is(abs(H), t._replace(v=np_map(t.v, "abs")), values=same_bits if kind == "real" else same_values)
    after = H.export_csr()
    assert all(same_bits(a, b) for a, b in zip(before, after))  # the operand is borrowed


def test_maps_keep_stored_zeros_and_special_values(gpu, base, handles):
    """what the restatements mean on the salt, spelled out"""
    t, H = base["real"], handles["real"]
    sg = H.signum().export_csr()[2]
    zero, nan = t.v == 0, np.isnan(t.v)
    assert same_bits(sg[zero], t.v[zero]) and same_bits(sg[nan], t.v[nan])  # +-0 and the NaN pass through
    assert set(sg[~zero & ~nan].tolist()) == {1.0, -1.0} and sg[t.v == 5e-324][0] == 1.0
    ng = H.negate().export_csr()[2]
    assert bits(ng[nan])[0] == bits(t.v[nan])[0] ^ SIGN  # the payload is kept
    im = H.imag().export_csr()[2]
    assert len(im) == len(t.v) and not np.any(bits(im))  # the same pattern, +0.0 everywhere
    z, HZ = base["complex"], handles["complex"]
    cj = HZ.conj().export_csr()[2]
    assert same_bits(cj.real, z.v.real) and same_bits(cj.imag, flip(z.v.imag.copy()))


@pytest.mark.parametrize("name", list(NARROW))
def test_maps_and_scaling_of_narrow_matrices(gpu, pkg, base, handles, name):
    torch = gpu
    rng = np.random.default_rng(11)
    for t, H in ((base[name], handles[name]), (narrow_complex(base[name]), None)):
        H = H or handle(torch, pkg, t)
        cplx = t.v.dtype == np.complex128
        for op, s in (("abs", None), ("signum", None), ("scale", 1.7)):
            assert_is(H.map(op, s), t._replace(v=np_map(t.v, op, s)))
        r, c = rng.standard_normal(t.nrows), rng.standard_normal(t.ncols)
        if cplx:
            r, c = r + 1j * rng.standard_normal(t.nrows), c + 1j * rng.standard_normal(t.ncols)
        assert_is(H.scale_rows_cols(r, c), t._replace(v=np_scale_rows_cols(t, r, c)))


def test_maps_on_a_row_block(gpu, base, block):
    B, sub = block
    for op, s in (("negate", None), ("signum", None), ("scale", -2.5), ("imag", None)):
        assert_is(B.map(op, s), sub._replace(v=np_map(sub.v, op, s)), values=same_values, row0=BLOCK[0], nrows_global=NR)


# ---- 2. magnitude and signum ----------------------------------------------------------------------------------------

def test_magnitude_is_ghcs_not_hypot(gpu, pkg):
    torch = gpu
    rng = np.random.default_rng(16)
    n = 10_007
    re = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
    im = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
    # a block of entries whose parts are of one size (where the rounding of the squares shows), and the corners
    re[:4000] = rng.standard_normal(4000)
    im[:4000] = rng.standard_normal(4000)
    corners = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 5e-324), (5e-324, 0.0), (5e-324, 5e-324),
               (-5e-324, 3e-323), (1e300, 1e300), (-1e300, 1e-300), (1e-300, 1e-300), (1e308, 1e308), (3.0, 4.0),
               (0.0, -2.5), (-2.5, 0.0), (2.2250738585072014e-308, 2.2250738585072014e-308), (1e-320, 1e-310),
               (1.0, 1e-20), (1e-160, 1e-170)]
    for k, (a, b) in enumerate(corners):
        re[5000 + k], im[5000 + k] = a, b
    keys = rng.choice(500 * 499, n, replace=False)
    t = csr_from_keys(500, 499, keys, pack(re, im))
    want = np_magnitude(t.v.real.copy(), t.v.imag.copy())
    hyp = np.hypot(t.v.real, t.v.imag)
    print("the restatement differs from np.hypot on %.1f %% of %d values" % (100 * np.mean(bits(want) != bits(hyp)), n))
    # it is a magnitude (within two units of hypot's), and it is not hypot's: a kernel that calls hypot cannot pass
    assert np.all((want == hyp) | (np.abs(want - hyp) <= 2 * np.spacing(hyp))) and np.mean(bits(want) != bits(hyp)) > 0.01
    H = handle(torch, pkg, t)
    assert_is(H.abs(), t._replace(v=pack(want, np.zeros(n))))
    assert_is(H.signum(), t._replace(v=np_map(t.v, "signum")))
    sg = H.signum().export_csr()[2]
    zero = (t.v.real == 0) & (t.v.imag == 0)
    assert zero.sum() == 4 and not np.any(bits(sg[zero]))  # 0 :+ 0, both +0.0
    # the moduli feed the filter and the reductions through the same function
    tol = float(np.median(want))
    assert_is(H.drop_small(tol), np_keep(t, ~(want <= tol)))
    assert same_bits(H.abs_max(1).cpu().numpy(), np.array([want[a:b].max() if b > a else 0.0
                                                          for a, b in zip(t.rp[:-1], t.rp[1:])]))


def test_magnitude_of_parts_that_are_not_finite(gpu, pkg):
    inf, nan = np.inf, np.nan
    pairs = [(inf, 1.0), (1.0, -inf), (inf, nan), (nan, inf), (-inf, -inf), (nan, 1.0), (1.0, nan), (nan, nan),
             (NAN_PAYLOAD, 0.0), (-inf, 0.0), (3.0, 4.0)]
    z = pack(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    t = csr_from_keys(3, 7, np.arange(len(pairs)) * 2, z)
    H = handle(gpu, pkg, t)
    got = H.abs().export_csr()[2]
    want = np.array([inf, inf, inf, inf, inf, nan, nan, nan, nan, inf, 5.0])
    assert not np.any(bits(got.imag.copy()))
    assert np.array_equal(np.isnan(got.real), np.isnan(want)) and np.array_equal(got.real[~np.isnan(want)], want[~np.isnan(want)])
    assert same_values(np.ascontiguousarray(got.real), np_magnitude(z.real.copy(), z.imag.copy()))
    # a NaN modulus is not <= tol: the entry stays; an infinite one stays for every finite tol
    assert H.drop_small(1e308).info()["nnz"] == len(pairs) - 1
    assert_is(H.signum(), t._replace(v=np_map(t.v, "signum")), values=same_values)


# ---- 3. scaling -----------------------------------------------------------------------------------------------------

def scaling_vectors(nrows, ncols, cplx):
    rng = np.random.default_rng(nrows + ncols)
    r = rng.standard_normal(nrows) * 10.0 ** rng.integers(-2, 3, nrows)
    c = rng.standard_normal(ncols) * 10.0 ** rng.integers(-2, 3, ncols)
    if cplx:
        r = r + 1j * rng.standard_normal(nrows)
        c = c + 1j * rng.standard_normal(ncols)
    return r, c


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_scaling_against_the_products(gpu, base, handles, kind):
    torch = gpu
    t, H = base[kind], handles[kind]
    r, c = scaling_vectors(NR, NC, kind == "complex")
    dr, dc = torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()
    before = H.export_csr()
    assert_is(H.scale_rows_cols(dr, None), t._replace(v=np_scale_rows_cols(t, r, None)), values=same_values)
    assert_is(H.scale_rows_cols(None, dc), t._replace(v=np_scale_rows_cols(t, None, c)), values=same_values)
    assert_is(H.scale_rows_cols(dr, dc), t._replace(v=np_scale_rows_cols(t, r, c)), values=same_values)
    assert_is(H.scale_rows_cols(r=r, c=c), t._replace(v=np_scale_rows_cols(t, r, c)), values=same_values)  # host arrays
    assert_is(H.scale_rows_cols(), t)  # neither: a copy, every bit
    ones = np.ones(NC) + (0j if kind == "complex" else 0.0)  # given, so multiplied with: inf * (1 :+ 0) has a NaN part
    assert_is(H.scale_rows_cols(c=list(np.ones(NC))), t._replace(v=np_scale_rows_cols(t, None, ones)), values=same_values)
    assert all(same_bits(a, b) for a, b in zip(before, H.export_csr()))
    if kind == "complex":  # real vectors on a complex handle are promoted, (x :+ 0)
        want = np_scale_rows_cols(t, r.real + 0j, None)
        assert_is(H.scale_rows_cols(torch.from_numpy(r.real.copy()).cuda()), t._replace(v=want), values=same_values)


def test_scaling_a_row_block(gpu, base, block):
    torch = gpu
    B, sub = block
    r, c = scaling_vectors(sub.nrows, NC, False)
    dr, dc = torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()
    for rr, cc, hr, hc in ((r, None, dr, None), (None, c, None, dc), (r, c, dr, dc), (None, None, None, None)):
        assert_is(B.scale_rows_cols(hr, hc), sub._replace(v=np_scale_rows_cols(sub, rr, cc)), values=same_values,
                  row0=BLOCK[0], nrows_global=NR)
    with pytest.raises(ValueError):
        B.scale_rows_cols(np.ones(NR))  # r has nrows_local entries


def test_scaling_keeps_the_sign_of_zero_where_two_products_with_diagonals_do_not(gpu, pkg):
    t = csr_from_keys(2, 2, [0, 1, 3], np.array([-0.0, 2.0, -0.0]))
    H = handle(gpu, pkg, t)
    got = H.scale_rows_cols(np.array([1.0, 3.0]), np.array([1.0, 1.0])).export_csr()[2]
    assert same_bits(got, np.array([-0.0, 2.0, -0.0]))


# ---- 4. filters -----------------------------------------------------------------------------------------------------

def np_nonzero(t):
    if t.v.dtype == np.complex128:
        return ~((t.v.real == 0) & (t.v.imag == 0))
    return ~(t.v == 0)


def test_a_matrix_minus_itself_dropped_of_zeros_is_zeros(gpu, base, handles):
    for name in ("mean7", "mean100"):
        t, H = base[name], handles[name]
        Z = H.lin(1.0, H, -1.0)
        assert Z.info()["nnz"] == len(t.ci)  # lin keeps the cancelled entries
        D = Z.drop_zeros()
        assert_is(D, Csr(t.nrows, t.ncols, np.zeros(t.nrows + 1, dtype=np.int64), t.ci[:0], t.v[:0]))


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_drop_zeros_on_a_mixture(gpu, base, handles, kind):
    t, H = base[kind], handles[kind]
    keep = np_nonzero(t)
    got = H.drop_zeros()
    assert_is(got, np_keep(t, keep))  # the order inside the rows is kept: the arrays are equal
    v = got.export_csr()[2]
    assert np.isnan(v.view(np.float64)).sum() == np.isnan(t.v.view(np.float64)).sum()  # NaN is kept
    if kind == "real":
        assert (~keep).sum() == 7 and not np.any(v == 0)  # -0.0 and +0.0 went
    else:
        z = t.v
        assert (~keep).sum() >= 3
        gone = z[~keep]
        assert np.any(np.signbit(gone.imag) & ~np.signbit(gone.real))  # (0, -0) went
        assert np.any((v.real == 0) & (v.imag == 5e-324))  # (0, 5e-324) stayed


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_drop_small_at_an_exact_modulus(gpu, base, handles, kind):
    t, H = base[kind], handles[kind]
    m = np_moduli(t)
    k = int(t.rp[LONG_ROW]) + 77
    tol = float(m[k])
    assert np.isfinite(tol) and tol > 0
    at = H.drop_small(tol)
    assert_is(at, np_keep(t, ~(m <= tol)))
    below = float(np.nextafter(tol, 0.0))
    under = H.drop_small(below)
    assert_is(under, np_keep(t, ~(m <= below)))
    # the entry itself: gone at its modulus, there just below it
    col = int(t.ci[k])
    row_at = np_rows(np_keep(t, ~(m <= tol)), LONG_ROW, LONG_ROW + 1)
    row_under = np_rows(np_keep(t, ~(m <= below)), LONG_ROW, LONG_ROW + 1)
    assert col not in row_at.ci and col in row_under.ci
    # |a| <= 0: on real values a == 0.  Not so on complex ones: GHC's magnitude (0 :+ 5e-324) is 0, because
    # exponent 0 = 0 is the larger exponent and the square of the unscaled 5e-324 vanishes; drop_zeros keeps that entry
    assert_is(H.drop_small(0.0), np_keep(t, ~(m <= 0.0)))
    if kind == "real":
        assert np.array_equal(m <= 0.0, ~np_nonzero(t))
    else:
        assert np.sum(m <= 0.0) == np.sum(~np_nonzero(t)) + 2
    assert_is(H.drop_small(np.inf), np_keep(t, np.isnan(m)))  # only what is not comparable stays


@pytest.mark.parametrize("name", list(NARROW))
def test_filters_of_narrow_matrices(gpu, pkg, base, handles, name):
    for t, H in ((base[name], handles[name]), (narrow_complex(base[name]), None)):
        H = H or handle(gpu, pkg, t)
        m = np_moduli(t)
        for q in (0.1, 0.5, 0.97):
            tol = float(np.quantile(m, q))
            assert_is(H.drop_small(tol), np_keep(t, ~(m <= tol)))
        assert_is(H.drop_zeros(), t)


def test_filters_on_a_row_block(gpu, base, block):
    B, sub = block
    assert_is(B.drop_zeros(), np_keep(sub, np_nonzero(sub)), row0=BLOCK[0], nrows_global=NR)
    m = np_moduli(sub)
    assert_is(B.drop_small(1.0), np_keep(sub, ~(m <= 1.0)), row0=BLOCK[0], nrows_global=NR)


# ---- 5. bands -------------------------------------------------------------------------------------------------------

BANDS = ((None, 0), (0, None), (None, -1), (1, None), (0, 0), (-3, 7), (5, -5), (1, 0),
         (None, None), (I64_MIN, I64_MAX), (-2 ** 62, 2 ** 62), (I64_MAX, None), (None, I64_MIN), (I64_MAX, I64_MAX),
         (None, NC + 5), (-(NR + 5), None), (None, -(NR + 5)), (NC + 5, None), (NC - 1, NC - 1), (-(NR - 1), -(NR - 1)),
         (-2500, 1700), (1000, 1003), (-4000, -3990))


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_bands_against_numpy_tall_and_wide(gpu, pkg, base, handles, kind):
    t, H = base[kind], handles[kind]
    w = np_transpose(t)  # 4 099 x 6 007
    W = handle(gpu, pkg, w)
    for lo, hi in BANDS:
        assert_is(H.band(lo, hi), np_band(t, lo, hi))
        if kind == "real" or (lo, hi) in ((-3, 7), (None, -1), (1, None)):
            assert_is(W.band(lo, hi), np_band(w, lo, hi))
    for k in (0, -1, 1, 7, -NR - 5, NC + 5):
        assert_is(H.tril(k), np_band(t, None, k))
        assert_is(H.triu(k), np_band(t, k, None))
    assert H.band(5, -5).info()["nnz"] == 0 and H.band(1, 0).info()["nnz"] == 0  # lo > hi: zeros of the shape


def test_the_three_pieces_hold_every_entry_once(gpu, base, handles):
    for kind in ("real", "complex"):
        t, H = base[kind], handles[kind]
        keys = []
        for lo, hi in ((None, -1), (0, 0), (1, None)):
            rp, ci, _ = H.band(lo, hi).export_csr()
            keys.append(np.repeat(np.arange(NR, dtype=np.int64), np.diff(rp)) * NC + ci)
        allkeys = np.concatenate(keys)
        assert len(allkeys) == len(t.ci) and np.array_equal(np.sort(allkeys), row_ids(t) * NC + t.ci)
        assert all(len(k) > 0 for k in keys)


def test_bands_of_a_row_block_use_the_global_row(gpu, base, block):
    B, sub = block
    for lo, hi in BANDS:
        assert_is(B.band(lo, hi), np_band(sub, lo, hi, row0=BLOCK[0]), row0=BLOCK[0], nrows_global=NR)
    local = np_band(sub, -3, 7)  # what a local row index would keep: something else
    assert not np.array_equal(local.rp, np_band(sub, -3, 7, row0=BLOCK[0]).rp)


@pytest.mark.parametrize("name", list(NARROW))
def test_bands_of_narrow_matrices(gpu, base, handles, name):
    t, H = base[name], handles[name]
    for lo, hi in ((None, 0), (0, None), (-3, 7), (-t.nrows // 2, t.ncols // 3), (0, 0), (-200, -100), (None, None)):
        assert_is(H.band(lo, hi), np_band(t, lo, hi))


# ---- 6. reductions --------------------------------------------------------------------------------------------------

def slices_of(t, axis):
    """(pointers, moduli) of the rows (axis 1) or the columns (axis 0)"""
    s = t if axis == 1 else np_transpose(t)
    return s.rp, np_moduli(s)


def check_abs_sums(got, ptr, m):
    worst = 0.0
    for i in range(len(ptr) - 1):
        part = m[ptr[i]:ptr[i + 1]]
        if len(part) == 0:
            assert bits(got[i:i + 1])[0] == 0, i  # +0.0
        elif np.isnan(part).any():
            assert np.isnan(got[i]), i
        elif np.isinf(part).any():
            assert got[i] == np.inf, i
        else:
            exact = math.fsum(part.tolist())
            bound = (len(part) + 4) * U * exact
            assert abs(got[i] - exact) <= bound, (i, got[i], exact, bound)
            worst = max(worst, abs(got[i] - exact) / (U * exact) if exact else 0.0)
    return worst


def expected_abs_max(ptr, m):
    out = np.zeros(len(ptr) - 1)
    for i in range(len(ptr) - 1):
        part = m[ptr[i]:ptr[i + 1]]
        if len(part):
            out[i] = np.nan if np.isnan(part).any() else part.max()
    return out


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_reductions_against_fsum(gpu, base, handles, kind, axis):
    t, H = base[kind], handles[kind]
    ptr, m = slices_of(t, axis)
    sums = H.abs_sums(axis)
    assert str(sums.device).startswith("cuda") and sums.dtype == gpu.float64 and sums.shape == (len(ptr) - 1,)
    got = sums.cpu().numpy()
    print("abs_sums axis %d %s: worst error %.2f u of the slice's sum" % (axis, kind, check_abs_sums(got, ptr, m)))
    assert same_bits(got, H.abs_sums(axis).cpu().numpy())  # two calls, the same bits
    mx = H.abs_max(axis).cpu().numpy()
    want = expected_abs_max(ptr, m)
    assert np.isnan(want).sum() >= 1  # a NaN in a slice is carried through
    assert same_values(mx, want) and same_bits(mx, H.abs_max(axis).cpu().numpy())


@pytest.mark.parametrize("name", list(NARROW))
def test_reductions_of_narrow_matrices(gpu, pkg, base, handles, name):
    for t, H in ((base[name], handles[name]), (narrow_complex(base[name]), None)):
        H = H or handle(gpu, pkg, t)
        for axis in (1, 0):
            ptr, m = slices_of(t, axis)
            got = H.abs_sums(axis).cpu().numpy()
            check_abs_sums(got, ptr, m)
            assert same_bits(got, H.abs_sums(axis).cpu().numpy())
            assert same_bits(H.abs_max(axis).cpu().numpy(), expected_abs_max(ptr, m))


def test_row_reductions_of_a_row_block(gpu, pkg, base, block):
    B, sub = block
    check_abs_sums(B.abs_sums(1).cpu().numpy(), sub.rp, np_moduli(sub))
    assert same_values(B.abs_max(1).cpu().numpy(), expected_abs_max(sub.rp, np_moduli(sub)))
    F = pkg._ffi
    for call in (lambda: B.abs_sums(0), lambda: B.abs_max(0), lambda: B.norm(1), lambda: B.norm("inf"),
                 lambda: B.norm("fro"), lambda: B.norm("max")):
        with pytest.raises(F.SparseLinearError) as e:
            call()
        assert e.value.status == F.SPL_ERROR_argument_missing


def exact_norms(t):
    m = np_moduli(t)
    cols = np_transpose(t)
    mc = np_moduli(cols)
    one = [(math.fsum(mc[a:b].tolist()), (b - a + 4) * U) for a, b in zip(cols.rp[:-1], cols.rp[1:])]
    inf = [(math.fsum(m[a:b].tolist()), (b - a + 4) * U) for a, b in zip(t.rp[:-1], t.rp[1:])]
    k = int(np.frexp(m.max())[1])
    parts = np.ascontiguousarray(t.v).view(np.float64)
    scaled = np.ldexp(parts, -k)  # exact
    fro = math.ldexp(math.sqrt(math.fsum((scaled * scaled).tolist())), k)
    return one, inf, fro, float(m.max())


def check_norms(H, t):
    one, inf, fro, mx = exact_norms(t)
    for which, slices in ((1, one), (float("inf"), inf)):
        got = H.norm(which)
        exact = max(s for s, _ in slices)
        bound = max(s * rel for s, rel in slices)  # every slice within its own bound: so is the largest
        assert abs(got - exact) <= bound, (which, got, exact, bound)
    got = H.norm("fro")
    assert abs(got - fro) <= (len(t.ci) + 4) * U * fro, (got, fro)
    assert H.norm("max") == mx
    assert H.norm() == got and H.norm("inf") == H.norm(float("inf")) and H.norm("1") == H.norm(1)  # and the same bits twice


def test_the_four_norms(gpu, pkg, base, handles):
    for name in ("mean7", "mean100", "mean1"):
        check_norms(handles[name], base[name])
        z = narrow_complex(base[name])
        check_norms(handle(gpu, pkg, z), z)
    # the base holds a NaN: every norm says so
    for kind in ("real", "complex"):
        assert all(np.isnan(handles[kind].norm(w)) for w in (1, "inf", "fro", "max"))
    # without it, an infinity
    t = base["real"]
    H = handle(gpu, pkg, np_keep(t, ~np.isnan(t.v)))
    assert all(H.norm(w) == np.inf for w in (1, "inf", "fro", "max"))


@pytest.mark.parametrize("scale", [1e200, 1e-200, 1.0, 5e-324, 1e308])
def test_frobenius_norm_of_badly_scaled_entries(gpu, pkg, scale):
    rng = np.random.default_rng(200)
    t = make_narrow("mean3")
    if scale == 5e-324:
        v = np.full(len(t.ci), 5e-324)  # the exact answer is sqrt(nnz) 2^-1074, far from 0
    elif scale == 1e308:
        v = np.full(len(t.ci), 1e308 / 128.0)  # sqrt(6409) 1e308 / 128 = 6.3e307: representable, the squares are not
    else:
        v = rng.standard_normal(len(t.ci)) * scale
    for t in (t._replace(v=v), t._replace(v=pack(v, v[::-1].copy()))):
        H = handle(gpu, pkg, t)
        _, _, fro, mx = exact_norms(t)
        got = H.norm("fro")
        assert np.isfinite(got) and got > 0 and abs(got - fro) <= (len(t.ci) + 4) * U * fro, (got, fro)
        assert H.norm("max") == mx


def test_an_empty_matrix(gpu, pkg, base, handles):
    E = handles["mean7"].band(1, 0)
    t = base["mean7"]
    assert E.info()["nnz"] == 0
    assert all(E.norm(w) == 0.0 for w in (1, "inf", "fro", "max"))
    for axis, n in ((1, t.nrows), (0, t.ncols)):
        for out in (E.abs_sums(axis), E.abs_max(axis)):
            assert out.shape == (n,) and not np.any(bits(out.cpu().numpy()))
    for X in (E.negate(), E.drop_zeros(), E.drop_small(1.0), E.band(None, None), E.scale_rows_cols(np.ones(t.nrows))):
        assert_is(X, Csr(t.nrows, t.ncols, np.zeros(t.nrows + 1, dtype=np.int64), t.ci[:0], t.v[:0]))
    Z = pkg.DeviceMatrix.ident(0)
    assert Z.norm("fro") == 0.0 and Z.abs_sums(1).shape == (0,) and Z.abs_sums(0).shape == (0,)
    assert Z.negate().info()["nnz"] == 0 and Z.drop_zeros().info()["nnz"] == 0 and Z.tril().info()["nnz"] == 0


# ---- 7. composition: the results are ordinary handles ---------------------------------------------------------------

def test_row_scaling_feeds_the_lu(gpu, pkg, O):
    """A = poisson3d(12) + 0.5 I, r = 1 / abs_max(rows): the factors of diag(r) A solve (diag(r) A) x = r * b, which is
    A x = b; the residual is formed with the oracle's product on the exported arrays of A"""
    torch = gpu
    U_ = pkg.umfpack
    n = 12 ** 3
    P = pkg.DeviceMatrix.synthetic("poisson3d", 12)
    A = P.lin(1.0, pkg.DeviceMatrix.ident(n), 0.5)
    r = 1.0 / A.abs_max(1)
    S = A.scale_rows_cols(r)
    assert np.all(np.abs(S.abs_max(1).cpu().numpy() - 1.0) <= 2 * U)  # every row's largest entry is 1 now, twice rounded
    f = U_.factorDevice(S, U_.analyzeDevice(S))
    b = np.random.default_rng(12).standard_normal(n)
    B = (r * torch.from_numpy(b).cuda())[None, :].contiguous()
    x = U_.linearSolveManyDevice_(f, U_.UmfpackNormal, None, B).cpu().numpy()[0]
    rp, ci, v = A.export_csr()
    res = O.axpy(O.csr_to_csc_tuple(n, n, rp, ci, v), x, -b)
    rel = float(np.linalg.norm(res) / np.linalg.norm(b))
    print("relative residual of A x = b: %.3g" % rel)
    assert rel <= 1e-10
    # and the pieces of A = L + D + U add up to A again, bit for bit
    back = A.tril(-1).lin(1.0, A.band(0, 0), 1.0).lin(1.0, A.triu(1), 1.0)
    assert all(same_bits(a, c) for a, c in zip(back.export_csr(), (rp, ci, v)))


# ---- 8. statuses on real handles ------------------------------------------------------------------------------------

def test_statuses_on_real_handles(gpu, pkg, base, handles):
    torch = gpu
    F = pkg._ffi
    L = F.lib()
    H, HZ = handles["real"], handles["complex"]

    def raw_map(X, op, scalar):
        h = C.c_void_p(0x1234)
        st = L.spl_matrix_map(X.handle, op, scalar, C.byref(h))
        assert st == 0 or not h.value  # *HC is cleared whenever the call is refused
        if st == 0:
            pkg.DeviceMatrix(h.value)  # owned, and freed
        return st

    assert raw_map(H, F.SPL_MAP_scale, (C.c_double * 2)(2.0, 0.5)) == F.SPL_ERROR_argument_missing  # imaginary, real handle
    assert raw_map(H, F.SPL_MAP_scale, (C.c_double * 2)(2.0, -0.0)) == 0
    assert raw_map(HZ, F.SPL_MAP_scale, (C.c_double * 2)(2.0, 0.5)) == 0
    assert raw_map(H, F.SPL_MAP_scale, None) == F.SPL_ERROR_argument_missing
    assert raw_map(H, F.SPL_MAP_negate, None) == 0  # the scalar is read by scale only
    assert raw_map(H, 7, None) == F.SPL_ERROR_argument_missing
    with pytest.raises(F.SparseLinearError):
        H.scale(1j)
    # reductions: a NULL output with a non-empty axis, codes, and a NULL result
    out = torch.zeros(NR, dtype=torch.float64, device="cuda")
    for axis in (0, 1):
        assert L.spl_matrix_reduce_dev(H.handle, 0, axis, None, None) == F.SPL_ERROR_argument_missing
        assert L.spl_matrix_reduce_dev(H.handle, 0, axis, C.c_void_p(out.data_ptr() + 4), None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_reduce_dev(H.handle, 2, 1, C.c_void_p(out.data_ptr()), None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_reduce_dev(H.handle, 0, 2, C.c_void_p(out.data_ptr()), None) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_norm(H.handle, F.SPL_NORM_fro, None) == F.SPL_ERROR_argument_missing
    r = C.c_double(-7.5)
    assert L.spl_matrix_norm(H.handle, 4, C.byref(r)) == F.SPL_ERROR_argument_missing and r.value == -7.5
    # filters
    h = C.c_void_p(0x1234)
    assert L.spl_matrix_filter(H.handle, F.SPL_KEEP_abs_above, (C.c_double * 1)(-1e-300), C.byref(h)) == \
        F.SPL_ERROR_argument_missing and not h.value
    assert L.spl_matrix_filter(H.handle, F.SPL_KEEP_abs_above, (C.c_double * 1)(float("nan")), C.byref(h)) == \
        F.SPL_ERROR_argument_missing
    assert L.spl_matrix_band(H.handle, 0, 0, None) == F.SPL_ERROR_argument_missing
    with pytest.raises(F.SparseLinearError):
        H.drop_small(-1.0)
    # the vectors, refused in Python before the call
    ok_r = torch.ones(NR, dtype=torch.float64, device="cuda")
    for bad in (ok_r.to(torch.float32), torch.ones(NR, dtype=torch.int64, device="cuda"), np.ones(NR, dtype=np.float32),
                ok_r.to(torch.complex128), torch.ones((NR, 1), dtype=torch.float64, device="cuda")):
        with pytest.raises(TypeError):
            H.scale_rows_cols(bad)
    for bad_r, bad_c in ((ok_r[:-1], None), (None, ok_r), (np.ones(NC), None)):
        with pytest.raises(ValueError):
            H.scale_rows_cols(bad_r, bad_c)
    with pytest.raises(TypeError):
        HZ.scale_rows_cols(ok_r.to(torch.float32))
