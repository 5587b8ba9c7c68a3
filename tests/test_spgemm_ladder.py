"""The SpGEMM ladder (tests/spgemm_ladder.py) has the properties tests/test_gpu_spgemm_bins.py leans on (no GPU, oracle
and scipy only): every column of B has the prescribed number of products and entries at every row count, the host
mirror of the dispatcher puts at least one column into every class, and the oracle's product of the ladder is a valid
matrix that scipy reproduces exactly on integer values."""
import collections
import time

import numpy as np
import pytest

import spgemm_ladder as L
from helpers import csc_tuple_to_scipy

# columns per class when no switch is set.  Up to 2^21 rows bin X goes with the heavy columns and the row-range kernel
# runs: it refuses x_products_l_length and few_2049 (entries of B), range_past (products) and hub (a row bucket);
# beyond, bin X runs on its own, in its two halves, and every heavy column goes to the dense accumulators
CLASSES_TO_2_21 = {"empty": 2, "S": 53, "M": 13, "X_as_range": 7, "L_range": 2, "L_dense_nb": 2, "L_dense_products": 1,
                   "L_dense_hub": 1}
CLASSES_BEYOND = {"empty": 2, "S": 53, "M": 13, "X_front": 2, "X_back": 5, "L_dense": 6}
ORDERED_CLASSES = {"small": {"empty": 2, "wave": 51, "group": 8, "listed": 20},
                   "large": {"empty": 2, "wave": 51, "group": 12, "listed": 16}}
# named columns whose class is the point of their being there
CLASS_OF = {"empty": "empty", "only_empty_columns": "empty", "s_edge": "S", "s_past": "M", "m_edge": "M", "ord_large_cap": "M",
            # (kMediumB = kSmallProducts = 256: a column of 257 entries of B is in bin X however few its products)
            "s_products_x_length": ("X_as_range", "X_back"), "few_257": ("X_as_range", "X_back"),
            "m_past": ("X_as_range", "X_front"), "x_edge_front": ("X_as_range", "X_front"),
            "x_long_b": ("X_as_range", "X_back"), "x_edge_back": ("X_as_range", "X_back"),
            "few_2048": ("X_as_range", "X_back"), "x_past": ("L_range", "L_dense"), "range_edge": ("L_range", "L_dense"),
            "x_products_l_length": ("L_dense_nb", "L_dense"), "few_2049": ("L_dense_nb", "L_dense"),
            "range_past": ("L_dense_products", "L_dense"), "hub": ("L_dense_hub", "L_dense")}
ORDERED_CLASS_OF = {"ord_wave_edge": ("wave", "wave"), "ord_wave_nb_past": ("group", "group"), "s_past": ("group", "group"),
                    "ord_small_cap": ("group", "group"), "ord_small_cap_past": ("listed", "group"),
                    "ord_small_nb": ("group", "group"), "ord_small_nb_past": ("listed", "group"),
                    "ord_large_nb": ("listed", "group"), "ord_large_nb_past": ("listed", "listed"),
                    "ord_large_cap": ("listed", "group"), "m_past": ("listed", "listed")}
# flags of the plan line per row count, no switch set: x_heavy = range, key32 of bins S / M / X
FLAGS = {4097: (1, "1/1/1"), 1 << 19: (1, "1/1/1"), (1 << 19) + 1: (1, "1/1/0"), 1 << 20: (1, "1/1/0"),
         (1 << 20) + 1: (1, "1/0/0"), (1 << 21) - 1: (1, "1/0/0"), 1 << 21: (1, "1/0/0"), (1 << 21) + 1: (0, "1/0/0"),
         1 << 23: (0, "1/0/0"), (1 << 23) + 1: (0, "0/0/0")}


@pytest.fixture(scope="module")
def ladders():
    return {m: L.ladder(m) for m in L.ROWS}


def test_row_counts_straddle_every_threshold():
    assert tuple(FLAGS) == L.ROWS
    for bound in (1 << 19, 1 << 20, 1 << 21, 1 << 23):
        assert bound in L.ROWS and bound + 1 in L.ROWS
    assert (1 << 21) - 1 in L.ROWS and min(L.ROWS) == 4097


@pytest.mark.parametrize("m", L.ROWS)
def test_table_is_what_numpy_recounts(O, ladders, m):
    A, B, table = ladders[m]
    assert A[0] == m and A[1] == B[0] and B[1] == len(table.names)
    assert O.check_matrix(A) == 0 and O.check_matrix(B) == 0
    lens = np.diff(A[2])
    for j, name in enumerate(table.names):
        ks = B[3][B[2][j]:B[2][j + 1]]
        assert table.nb[j] == len(ks) and table.products[j] == lens[ks].sum(), name
    got = {name: (int(p), int(q)) for name, p, q in zip(table.names, table.products, table.nb)}
    assert got["empty"] == (0, 0) and got["only_empty_columns"] == (0, 300) and got["s_past"] == (257, 1)
    for name, products, nb in L.CASES:
        assert got[name][0] == products and (nb is None or got[name][1] == nb), name
        j = table.names.index(name)
        k = B[3][B[2][j + 1] - 1]          # the last entry of the column: A's last column, one entry, in the last row
        assert k == A[1] - 1 and lens[k] == 1 and A[3][-1] == m - 1
    assert got["range_edge"][1] <= 2048 and got["range_past"][1] <= 2048 and got["hub"][1] == 2048
    assert table.names.count("ordinary") == L.N_ORDINARY
    ordinary = np.array([n == "ordinary" for n in table.names])
    assert table.products[ordinary].min() >= 1 and table.products[ordinary].max() <= 256 and table.nb[ordinary].max() <= 12
    # A: many columns of 0, 1 and 16 entries, some of 1 000, long ones with the first and the last row
    count = collections.Counter(lens.tolist())
    assert count[0] == 2300 and count[16] == 400 and count[1000] == 8 and count[L.LONG] == 130 and count[257] == 1
    for c in np.flatnonzero(lens == L.LONG):
        assert A[3][A[2][c]] == 0 and A[3][A[2][c + 1] - 1] == m - 1
    assert len(A[3]) < 1_500_000 and 1_000_000 < table.products.sum() < 4_000_000
    # the crowded group: 2 400 columns inside a window of max(1, m // 4096) rows
    window = max(1, m // 4096)
    crowded = L._build_a(np.random.default_rng([m, 0]), m)[3]["crowded"]   # the builder's first draws: the same columns
    assert len(crowded) == 2400 and np.all(lens[crowded] == min(window, 8))
    assert all(A[3][A[2][c + 1] - 1] < window for c in crowded)
    j = table.names.index("hub")
    assert np.count_nonzero(np.isin(B[3][B[2][j]:B[2][j + 1]], crowded)) == L.HUB[0]
    assert not np.array_equal(A[4], np.round(A[4])) and not np.array_equal(B[4], np.round(B[4]))


@pytest.mark.parametrize("m", L.ROWS)
def test_mirror_puts_a_column_into_every_class(ladders, m):
    A, B, table = ladders[m]
    beyond = m > 1 << 21
    cls = L.classes(A, B)
    assert dict(collections.Counter(cls)) == (CLASSES_BEYOND if beyond else CLASSES_TO_2_21)
    for name, want in CLASS_OF.items():
        want = want if isinstance(want, str) else want[1 if beyond else 0]
        assert cls[table.names.index(name)] == want, name
    for t, shape in enumerate(("small", "large")):
        oc = L.ordered_classes(A, B, shape)
        assert dict(collections.Counter(oc)) == ORDERED_CLASSES[shape]
        for name, want in ORDERED_CLASS_OF.items():
            assert oc[table.names.index(name)] == want[t], (name, shape)
    # the plan of the default form: flags from the row count, counts from the classes
    plan = L.plan(A, B)
    heavy, key32 = FLAGS[m]
    assert (plan["rows"], plan["single_pass"], plan["ordered"], plan["shape"]) == (m, 1, 0, "none")
    assert (plan["x_heavy"], plan["range"], plan["key32"]) == (heavy, heavy, key32)
    counts = (plan["medium"], plan["xlarge"], plan["xback"], plan["heavy"], plan["dense"])
    assert counts == ((13, 2, 5, 6, 6) if beyond else (13, 0, 0, 13, 4))


def test_mirror_of_the_forced_forms(ladders):
    """the switches at 4 097 rows, where every one of them is honoured, and at 2^21 + 1, where the ordered form is
    refused and bin X and the dense accumulators are the default"""
    def counts(m, form, single_pass=None):
        p = L.plan(*ladders[m][:2], form, single_pass)
        return (p["ordered"], p["shape"], p["x_heavy"], p["range"], p["key32"], p["medium"], p["xlarge"], p["xback"],
                p["heavy"], p["dense"])
    small, big = 4097, (1 << 21) + 1
    assert counts(small, {}) == (0, "none", 1, 1, "1/1/1", 13, 0, 0, 13, 4)
    # ordered: its own kernel takes `wave` and `group`; of the 20 / 16 listed columns 13 are heavy
    assert counts(small, {"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "small"}) == \
        (1, "small", 1, 1, "1/1/1", 7, 0, 0, 13, 4)
    assert counts(small, {"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "large"}) == \
        (1, "large", 1, 1, "1/1/1", 3, 0, 0, 13, 4)
    assert counts(small, {"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "large"}, single_pass=0)[:2] == (0, "none")
    assert counts(small, {"SPL_SPGEMM_ORDERED": "0"}) == counts(small, {})
    assert counts(small, {"SPL_SPGEMM_TWO_PASS": "1"}) == counts(small, {})
    assert L.plan(*ladders[small][:2], {"SPL_SPGEMM_TWO_PASS": "1"})["single_pass"] == 0
    assert counts(small, {"SPL_SPGEMM_SPLIT_KEYS": "1"}) == (0, "none", 1, 1, "0/0/0", 13, 0, 0, 13, 4)
    assert counts(small, {"SPL_SPGEMM_X_AS_HEAVY": "0"}) == (0, "none", 0, 1, "1/1/1", 13, 2, 5, 6, 4)
    assert counts(small, {"SPL_SPGEMM_RANGE": "0"}) == (0, "none", 1, 0, "1/1/1", 13, 0, 0, 13, 13)
    assert counts(small, {"SPL_SPGEMM_X_AS_HEAVY": "0", "SPL_SPGEMM_SPLIT_KEYS": "1"}) == \
        (0, "none", 0, 1, "0/0/0", 13, 2, 5, 6, 4)
    assert counts(small, {"SPL_SPGEMM_TWO_PASS": "1", "SPL_SPGEMM_RANGE": "0"}) == (0, "none", 1, 0, "1/1/1", 13, 0, 0, 13, 13)
    for form in ({}, {"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "large"}, {"SPL_SPGEMM_ORDERED": "0"},
                 {"SPL_SPGEMM_TWO_PASS": "1"}, {"SPL_SPGEMM_X_AS_HEAVY": "0"}, {"SPL_SPGEMM_RANGE": "0"}):
        assert counts(big, form) == (0, "none", 0, 0, "1/0/0", 13, 2, 5, 6, 6), form
    assert counts(big, {"SPL_SPGEMM_SPLIT_KEYS": "1"}) == (0, "none", 0, 0, "0/0/0", 13, 2, 5, 6, 6)
    # the ordered form is taken up to 2^21 - 1 rows
    assert counts((1 << 21) - 1, {"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "small"})[:2] == (1, "small")
    assert counts(1 << 21, {"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "small"})[:2] == (0, "none")


def test_parse_plan():
    text = ("[spgemm] products, scan, totals                0.123 ms\n"
            "[spgemm] plan: rows=4097 single_pass=1 ordered=1 shape=small x_heavy=1 range=1 key32=1/1/0 medium=7 xlarge=0 "
            "xback=5 heavy=13 dense=4\n[spgemm] heavy columns: 13, of them 4 through the dense accumulators\n")
    assert L.parse_plan(text) == [{"rows": 4097, "single_pass": 1, "ordered": 1, "shape": "small", "x_heavy": 1, "range": 1,
                                   "key32": "1/1/0", "medium": 7, "xlarge": 0, "xback": 5, "heavy": 13, "dense": 4}]
    assert L.parse_plan("") == []


@pytest.mark.parametrize("m", [4097, (1 << 21) + 1])
def test_oracle_equals_scipy_on_integer_values(O, m):
    """the independent check of test_mm_vs_scipy_independent, on this structure: integer values, every sum exact"""
    A, B, _ = L.ladder(m, values="int")
    assert np.array_equal(A[4], np.round(A[4])) and np.all(A[4] != 0) and np.all(B[4] != 0)
    C = O.mm(A, B)
    assert O.check_matrix(C) == 0
    assert L.equals_scipy_product(C, csc_tuple_to_scipy(A) @ csc_tuple_to_scipy(B))
    assert 0 < np.count_nonzero(C[4] == 0) < len(C[4]) // 50   # sums that cancel stay stored (Sparse.hs:691-702)


@pytest.mark.parametrize("m", [4097, (1 << 23) + 1])
def test_oracle_product_of_the_ladder(O, ladders, m):
    A, B, table = ladders[m]
    t0 = time.perf_counter()
    C = O.mm(A, B)
    print("oracle mm at m = %d: %.2f s, %d products, %d entries" % (m, time.perf_counter() - t0, table.products.sum(), C[2][-1]))
    assert O.check_matrix(C) == 0
    lens = dict(zip(table.names, np.diff(C[2]).tolist()))
    # distinct rows: as many entries as products, on both sides of the complex kernel's chunks of 512
    assert [lens[k] for k in ("c_512", "c_513", "c_1024", "c_1025")] == [512, 513, 1024, 1025]
    # products that merge: the hub column sums 2 000 and more terms per row of its window
    j = table.names.index("hub")
    assert lens["hub"] < table.products[j] - 1900
    assert lens["range_edge"] <= 1 << 19 and (m > 1 << 19 or lens["range_edge"] == m)
    for name, _, _ in L.CASES:      # every edge column reaches the last row
        j = table.names.index(name)
        assert C[3][C[2][j + 1] - 1] == m - 1, name
    Cz = O.mm_z(*L.ladder(m, complex=True)[:2])
    assert np.array_equal(Cz[2], C[2]) and np.array_equal(Cz[3], C[3]) and np.count_nonzero(Cz[4].imag) > 0
