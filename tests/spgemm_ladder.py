"""A deterministic "ladder" of SpGEMM inputs and a host mirror of the dispatcher of csrc/spgemm.hip.

A plain module: numpy only, no fixtures, no GPU, nothing from the library under test.  `ladder(m, seed)` builds oracle
CSC tuples A (m x n) and B (n x p) in which every column of B has a PRESCRIBED number of products and of entries: one
column on each side of every comparison the dispatcher makes (bin_of's 256 / 2 048 / 4 096 products and 256 / 2 048
entries of B, the ordered form's column shapes, the row-range kernel's refusals).  `plan(A, B, form, single_pass)`
repeats the dispatcher's decisions on the host, from the code, and returns what its `[spgemm] plan:` line (printed
under SPL_SPGEMM_TIMING) must say; `parse_plan` reads that line.  tests/test_spgemm_ladder.py checks the builder and
the mirror, tests/test_gpu_spgemm_bins.py runs the kernels against them.

The row count m costs nothing (A has a few thousand columns whatever m is), so the same ladder serves every row-count
regime: 32-bit or split sort keys per bin, bin X with the heavy columns or on its own, the row-range kernel on or off."""
import collections
import re

import numpy as np

# ---- the dispatcher's constants (csrc/spgemm.hip) -----------------------------------------------------------------
K_SMALL = 256                           # kSmallProducts: products and entries of B of the one-wavefront kernel
K_MEDIUM, K_MEDIUM_B = 2048, 256        # kMediumProducts, kMediumB
K_LARGE, K_LARGE_B = 4096, 2048         # kLargeProducts, kLargeB
ORD_WAVE = (256, 64)                    # kOrdWaveCap, kOrdWaveNb: a column one wavefront of the ordered kernel takes
ORD_SHAPES = {"small": (1536, 96), "large": (2048, 128)}  # kOrdCap*, kOrdPNb*
ORD_ROWS = 1 << 21                      # the ordered form needs nrowsA < 2^kOrdMaxRowBits
HEAVY_ROWS = 1 << 21                    # x_heavy and the row-range kernel need nrowsA <= 2^21
KEY32_ROWS = {"s": 1 << 23, "m": 1 << 20, "x": 1 << 19}   # packed keys: nrowsA <= 2^(31 - log2(products of the bin))
RNG_NB, RNG_CAP, RNG_BUCKETS, RNG_MAX_RANGES, RNG_MAX_PRODUCTS = 2048, 2048, 4096, 1024, 1 << 19

# row counts on both sides of every comparison with nrowsA: key32_x, key32_m, the ordered form / x_heavy / row-range
# kernel, key32_s
ROWS = (4097, 1 << 19, (1 << 19) + 1, 1 << 20, (1 << 20) + 1, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, 1 << 23, (1 << 23) + 1)

LONG = 4096                             # length of a long column of A
# groups of columns of A: name, how many, length (None: see _build_a)
GROUPS = (("empty", 2300, 0), ("one", 700, 1), ("sixteen", 400, 16), ("thousand", 8, 1000), ("crowded", 2400, None),
          ("long", 130, LONG), ("disjoint", 3, None), ("p257", 1, 257))
DISJOINT = (512, 512, 1)                # three columns with no row in common: 512, 513, 1 024, 1 025 entries of C

# columns of B with a prescribed (products, entries of B); every one of them ends in A's last column, whose single
# entry is in row m - 1: the last product of the column — the largest tie-break value — lies in the last row
CASES = (("s_edge", 256, 256), ("s_products_x_length", 256, 257), ("m_edge", 2048, 256), ("m_past", 2049, 8),
         ("x_long_b", 2048, 257), ("x_edge_front", 4096, 256), ("x_edge_back", 4096, 2048), ("x_past", 4097, 9),
         ("x_products_l_length", 4096, 2049), ("few_257", 40, 257), ("few_2048", 40, 2048), ("few_2049", 40, 2049),
         ("range_edge", 1 << 19, 160), ("range_past", (1 << 19) + 1, None),
         ("ord_small_cap", 1536, 90), ("ord_small_cap_past", 1537, 90), ("ord_small_nb", 600, 96),
         ("ord_small_nb_past", 600, 97), ("ord_large_nb", 600, 128), ("ord_large_nb_past", 600, 129),
         ("ord_large_cap", 2048, 100), ("ord_wave_edge", 256, 64), ("ord_wave_nb_past", 256, 65))
HUB = (2000, 48)                        # the hub column: 2 000 crowded columns and 48 long ones, 2 048 entries of B
N_ORDINARY = 50

Table = collections.namedtuple("Table", "names products nb")


def _cplx(re, im):
    v = np.empty(len(re), dtype=np.complex128)
    v.real = re
    v.imag = im
    return v


def _values(rng, k, values, complex):
    def draw():
        if values == "int":  # no zeros: every stored entry of the product is then a sum of nonzero integers
            return rng.choice(np.array([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0]), k)
        assert values == "normal"
        return rng.standard_normal(k)
    return _cplx(draw(), draw()) if complex else draw()


def _build_a(rng, m):
    """the pattern of A: (pointers, indices, {group: its column numbers}).  The groups are scattered over the column
    numbers (a column of B meets them in mixed order); the last column holds row m - 1 alone."""
    assert m >= LONG + 1
    n = sum(g[1] for g in GROUPS) + 1
    perm = rng.permutation(n - 1)
    window = max(1, m // 4096)           # the crowded group's rows: inside the first of the range kernel's row buckets
    crowded_len = min(window, 8)
    cols, rows, at = {}, [None] * n, 0
    for name, count, length in GROUPS:
        ids = np.sort(perm[at:at + count])
        at += count
        cols[name] = ids
        if name == "disjoint":
            d = rng.choice(m, sum(DISJOINT), replace=False)
            cut = np.cumsum((0,) + DISJOINT)
            for t, c in enumerate(ids):
                rows[c] = np.sort(d[cut[t]:cut[t + 1]])
            continue
        for c in ids:
            if name == "crowded":
                r = rng.choice(window, crowded_len, replace=False)
            elif name == "long":        # row 0, row m - 1 and 4 094 rows between them
                r = np.concatenate([[0], 1 + rng.choice(m - 2, LONG - 2, replace=False), [m - 1]])
            elif name == "p257":        # one column of 257 entries, the last of them in row m - 1
                r = np.concatenate([rng.choice(m - 1, length - 1, replace=False), [m - 1]])
            else:
                r = rng.choice(m, length, replace=False)
            rows[c] = np.sort(r)
    rows[n - 1] = np.array([m - 1])
    cols["tail"] = np.array([n - 1])
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return n, p, np.concatenate(rows).astype(np.int64), cols


def _pick(rng, cols, products, nb):
    """columns of A whose lengths sum to `products`, `nb` of them (any number if None), the last one A's last column"""
    rest, take = products - 1, {}
    for name, length in (("long", LONG), ("thousand", 1000), ("sixteen", 16), ("one", 1)):
        take[name] = min(rest // length, len(cols[name]))
        rest -= take[name] * length
    assert rest == 0
    used = 1 + sum(take.values())
    if nb is not None:
        while take["sixteen"] > 0 and used + 15 <= nb and take["one"] + 16 <= len(cols["one"]):
            take["sixteen"] -= 1        # a column of 16 for 16 columns of 1: fewer empty columns to fill up with
            take["one"] += 16
            used += 15
        take["empty"] = nb - used
        assert 0 <= take["empty"] <= len(cols["empty"])
    sel = [cols["tail"]] + [rng.choice(cols[g], k, replace=False) for g, k in take.items() if k]
    return np.sort(np.concatenate(sel))


def ladder(m, seed=0, values="normal", complex=False):
    """(A, B, table): oracle CSC tuples A (m x n), B (n x p) and, per column of B, its name, its number of products and
    its number of entries.  The patterns depend on (m, seed) only; `values` is "normal" (the order of summation shows
    in the bits) or "int" (every sum exact); complex=True gives both factors complex values."""
    rng = np.random.default_rng([int(m), int(seed)])
    n, ap, ai, cols = _build_a(rng, m)
    lens = np.diff(ap)
    named = [("empty", np.zeros(0, dtype=np.int64)),
             ("only_empty_columns", np.sort(rng.choice(cols["empty"], 300, replace=False))),
             ("s_past", cols["p257"]),
             ("hub", np.sort(np.concatenate([rng.choice(cols["crowded"], HUB[0], replace=False),
                                             rng.choice(cols["long"], HUB[1], replace=False)])))]
    d = cols["disjoint"]
    named += [("c_512", d[[0]]), ("c_513", np.sort(d[[0, 2]])), ("c_1024", np.sort(d[[0, 1]])), ("c_1025", np.sort(d))]
    named += [(name, _pick(rng, cols, products, nb)) for name, products, nb in CASES]
    light = np.concatenate([cols["one"], cols["sixteen"], cols["empty"][:200]])
    for _ in range(N_ORDINARY):         # one to twelve entries, at least one product
        sel = np.concatenate([rng.choice(cols["one"], 1), rng.choice(light, int(rng.integers(0, 12)), replace=False)])
        named.append(("ordinary", np.unique(sel)))
    order = rng.permutation(len(named))
    named = [named[t] for t in order]
    nb = np.array([len(s) for _, s in named], dtype=np.int64)
    bp = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    bi = np.concatenate([s for _, s in named]).astype(np.int64)
    products = np.array([int(lens[s].sum()) for _, s in named], dtype=np.int64)
    A = (int(m), n, ap, ai, _values(rng, len(ai), values, complex))
    B = (n, len(named), bp, bi, _values(rng, len(bi), values, complex))
    return A, B, Table([name for name, _ in named], products, nb)


# ---- the dispatcher, on the host ----------------------------------------------------------------------------------

def products_and_nb(A, B):
    """per column of B: the number of products (sum of the lengths of the columns of A it selects) and of entries"""
    lens = np.diff(np.asarray(A[2], dtype=np.int64))
    run = np.concatenate([[0], np.cumsum(lens[np.asarray(B[3], dtype=np.int64)])])
    bp = np.asarray(B[2], dtype=np.int64)
    return run[bp[1:]] - run[bp[:-1]], np.diff(bp)


def bin_of(products, nb):
    """bin_of of csrc/spgemm.hip on arrays: 0 empty, 1 S, 2 M, 3 X, 4 L"""
    b = np.full(len(products), 4)
    b[(products <= K_LARGE) & (nb <= K_LARGE_B)] = 3
    b[(products <= K_MEDIUM) & (nb <= K_MEDIUM_B)] = 2
    b[(products <= K_SMALL) & (nb <= K_SMALL)] = 1
    b[products == 0] = 0
    return b


def range_refusal(A, B, j, products, nb):
    """why spgemm_range_kernel hands column j to the dense accumulators: "nb", "products", "hub", "ranges" or None"""
    if nb > RNG_NB:
        return "nb"
    if products > RNG_MAX_PRODUCTS:
        return "products"
    shift = 0
    while (RNG_BUCKETS << shift) < A[0]:
        shift += 1
    ap, ai = A[2], A[3]
    ks = B[3][B[2][j]:B[2][j + 1]]
    rows = np.concatenate([ai[ap[k]:ap[k + 1]] for k in ks]) if len(ks) else np.zeros(0, dtype=np.int64)
    hist = np.bincount(rows >> shift, minlength=RNG_BUCKETS)
    if hist.max() > RNG_CAP:
        return "hub"
    run = np.concatenate([[0], np.cumsum(hist)])
    nranges, start = 0, 0
    while start < RNG_BUCKETS:             # consecutive buckets while their products fit RNG_CAP
        if nranges >= RNG_MAX_RANGES:
            return "ranges"
        start = int(np.searchsorted(run, run[start] + RNG_CAP, side="right")) - 1
        nranges += 1
    return None


def classes(A, B):
    """per column of B, its class when no switch is set: empty, S, M, then up to 2^21 rows (bin X goes with the heavy
    columns, the row-range kernel runs) X_as_range, L_range and, for a refused column, L_dense_nb, L_dense_products,
    L_dense_hub; beyond 2^21 rows X_front, X_back and L_dense"""
    products, nb = products_and_nb(A, B)
    b = bin_of(products, nb)
    heavy_rows = A[0] <= HEAVY_ROWS
    out = []
    for j in range(len(b)):
        if b[j] < 3:
            out.append(("empty", "S", "M")[b[j]])
        elif b[j] == 3 and not heavy_rows:
            out.append("X_front" if nb[j] <= K_MEDIUM_B else "X_back")
        elif not heavy_rows:
            out.append("L_dense")
        else:
            why = range_refusal(A, B, j, products[j], nb[j])
            out.append(("X_as_" if b[j] == 3 else "L_") + ("range" if why is None else "dense_" + why))
    return out


def ordered_classes(A, B, shape):
    """per column of B, its class in the ordered form: empty, wave, group (the ordered kernel's own paths), listed"""
    products, nb = products_and_nb(A, B)
    cap, ord_nb = ORD_SHAPES[shape]
    return ["empty" if n == 0 else "wave" if n <= ORD_WAVE[0] and q <= ORD_WAVE[1] else
            "group" if n <= cap and q <= ord_nb else "listed" for n, q in zip(products, nb)]


def plan(A, B, form=None, single_pass=None):
    """what the `[spgemm] plan:` line of spgemm_device(A, B) must say under the environment `form`.  single_pass
    depends on the free device memory: pass what the line itself reports (None: the products fit, taken for granted)"""
    form = form or {}
    on = lambda key: form.get(key, "")[:1] == "1"
    off = lambda key: form.get(key, "")[:1] == "0"
    m = int(A[0])
    products, nb = products_and_nb(A, B)
    total = int(products.sum())
    x_heavy = not off("SPL_SPGEMM_X_AS_HEAVY") and m <= HEAVY_ROWS
    two_pass, split = on("SPL_SPGEMM_TWO_PASS"), on("SPL_SPGEMM_SPLIT_KEYS")
    if single_pass is None:
        single_pass = total > 0
    single_pass = bool(single_pass) and not two_pass and total > 0
    ordered, shape = False, "none"
    if not off("SPL_SPGEMM_ORDERED") and m < ORD_ROWS and not two_pass and not split and single_pass:
        wide = products > 2 * ORD_WAVE[0]
        share = {k: int(products[wide & (products <= c) & (nb <= q)].sum()) for k, (c, q) in ORD_SHAPES.items()}
        ordered = on("SPL_SPGEMM_ORDERED") or 2.0 * share["large"] >= total
        large = (share["large"] - share["small"]) > 0.08 * total
        if "SPL_SPGEMM_ORDERED_SHAPE" in form:
            large = form["SPL_SPGEMM_ORDERED_SHAPE"][:1] == "l"
        if ordered:
            shape = "large" if large else "small"
    b = bin_of(products, nb)
    if x_heavy:
        b[b == 3] = 4
    if ordered:
        cap, ord_nb = ORD_SHAPES[shape]
        own = (products <= cap) & (nb <= ord_nb)
        b = np.where(products == 0, 0, np.where(own, 1, np.maximum(b, 2)))
    heavy = np.flatnonzero(b == 4)
    use_range = len(heavy) > 0 and not off("SPL_SPGEMM_RANGE") and m <= HEAVY_ROWS
    dense = len(heavy)
    if use_range:
        dense = sum(range_refusal(A, B, j, products[j], nb[j]) is not None for j in heavy)
    return {"rows": m, "single_pass": int(single_pass), "ordered": int(ordered), "shape": shape, "x_heavy": int(x_heavy),
            "range": int(use_range), "key32": "/".join(str(int(not split and m <= KEY32_ROWS[k])) for k in "smx"),
            "medium": int(np.count_nonzero(b == 2)), "xlarge": int(np.count_nonzero((b == 3) & (nb <= K_MEDIUM_B))),
            "xback": int(np.count_nonzero((b == 3) & (nb > K_MEDIUM_B))), "heavy": len(heavy), "dense": int(dense)}


PLAN_KEYS = ("rows", "single_pass", "ordered", "shape", "x_heavy", "range", "key32", "medium", "xlarge", "xback", "heavy",
             "dense")


def parse_plan(stderr):
    """the plan lines in what a product wrote to stderr, each as a dict with plan()'s keys"""
    out = []
    for line in stderr.splitlines():
        if not line.startswith("[spgemm] plan:"):
            continue
        d = dict(re.findall(r"(\w+)=(\S+)", line))
        assert tuple(d) == PLAN_KEYS, line
        out.append({k: v if k in ("shape", "key32") else int(v) for k, v in d.items()})
    return out


def equals_scipy_product(C, ref):
    """the tuple C against scipy's product of the same factors, exactly.  scipy drops the sums that cancel to zero, mm
    keeps them stored: the stored zeros of C must be just the positions scipy does not have"""
    ref = ref.tocsc()
    ref.sort_indices()
    keep = C[4] != 0
    col = np.repeat(np.arange(C[1]), np.diff(C[2]))[keep]
    p = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=C[1]))])
    return bool(ref.shape == (C[0], C[1]) and np.all(ref.data != 0) and np.array_equal(ref.indptr, p)
                and np.array_equal(ref.indices, C[3][keep]) and np.array_equal(ref.data, C[4][keep]))
