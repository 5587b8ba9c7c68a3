"""SpGEMM (csrc/spgemm.hip, csrc/spgemm_z.hip) on the ladder of tests/spgemm_ladder.py: a column of B on each side of
every bin edge, at a row count on each side of every threshold the dispatcher compares nrowsA with, in the default
form and under every switch that production's large matrices take by themselves (bin X on its own, split sort keys,
the dense accumulators without the row-range kernel).

Every test computes C = A B, asserts structure and values bit for bit against the oracle (no tolerance) and the format
invariants, and reads the `[spgemm] plan:` line the product prints under SPL_SPGEMM_TIMING: the form, the flags and the
number of columns per kernel list must be what the host mirror (spgemm_ladder.plan) derives from the row count and the
switches — a column that was listed for another kernel, or a flag that came out otherwise, fails the test.  (The line
shows the dispatcher's decisions, not the template instance launched under them: that a branch under a flag launches
the right instance is guarded by the bit-exact values alone.)  single_pass depends on the free device memory, so the
mirror is given the value the line reports, and what rests on it is asserted only when the line reports it."""
import numpy as np
import pytest

import complex_handle_cases as K
import spgemm_ladder as L
from helpers import csc_tuple_to_scipy, mat_to_tuple, tuple_to_mat, tuples_equal

pytestmark = pytest.mark.gpu

SWITCHES = ("SPL_SPGEMM_ORDERED", "SPL_SPGEMM_ORDERED_SHAPE", "SPL_SPGEMM_TWO_PASS", "SPL_SPGEMM_SPLIT_KEYS",
            "SPL_SPGEMM_X_AS_HEAVY", "SPL_SPGEMM_RANGE", "SPL_SPGEMM_RING", "SPL_SPGEMM_ORD_CAP", "SPL_SPGEMM_STAMPS")
SMALL, BELOW, BEYOND = 4097, (1 << 21) - 1, (1 << 21) + 1
ORDERED_FORMS = ({"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "small"},
                 {"SPL_SPGEMM_ORDERED": "1", "SPL_SPGEMM_ORDERED_SHAPE": "large"})
OTHER_FORMS = ({"SPL_SPGEMM_ORDERED": "0"}, {"SPL_SPGEMM_TWO_PASS": "1"}, {"SPL_SPGEMM_SPLIT_KEYS": "1"},
               {"SPL_SPGEMM_X_AS_HEAVY": "0"}, {"SPL_SPGEMM_RANGE": "0"},
               {"SPL_SPGEMM_X_AS_HEAVY": "0", "SPL_SPGEMM_SPLIT_KEYS": "1"},
               {"SPL_SPGEMM_TWO_PASS": "1", "SPL_SPGEMM_RANGE": "0"})
# the ordered form is refused from 2^21 rows on: it is forced at 4 097 and at 2^21 - 1 rows, the others at 4 097 and 2^21 + 1
FORCED = [(m, f) for f in ORDERED_FORMS for m in (SMALL, BELOW)] + [(m, f) for f in OTHER_FORMS for m in (SMALL, BEYOND)]
# bin X on its own where production never has it: its packed keys at their largest legal row (row << 12 | t at 2^19
# rows), its split keys just beyond and at the last row count of the row-range kernel
FORCED += [(m, {"SPL_SPGEMM_X_AS_HEAVY": "0"}) for m in (1 << 19, (1 << 19) + 1, 1 << 21)]


def form_id(v):
    if isinstance(v, dict):
        return "+".join("%s=%s" % (k[len("SPL_SPGEMM_"):].lower(), x) for k, x in v.items())
    return str(v)


@pytest.fixture(scope="module")
def truth(O):
    """m -> (A, B, table, oracle's A B): built once per row count, shared by every test, never written to"""
    cache = {}

    def get(m):
        if m not in cache:
            A, B, table = L.ladder(m)
            cache[m] = (A, B, table, O.mm(A, B))
        return cache[m]
    return get


@pytest.fixture
def switches(monkeypatch):
    """no SpGEMM switch set but SPL_SPGEMM_TIMING (which prints the plan line); returns a setter for a form"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPL_SPGEMM_TIMING", "1")

    def use(form):
        for k, v in form.items():
            monkeypatch.setenv(k, v)
    return use


def planned(capfd, call):
    """call(), and the one plan line it printed"""
    capfd.readouterr()
    out = call()
    plans = L.parse_plan(capfd.readouterr().err)
    assert len(plans) == 1, plans
    return out, plans[0]


def check_product(pkg, O, capfd, A, B, ref, form):
    C, plan = planned(capfd, lambda: pkg.mm(tuple_to_mat(pkg, A), tuple_to_mat(pkg, B)))
    C = mat_to_tuple(C)
    print("plan:", plan)
    assert tuples_equal(C, ref)
    assert O.check_matrix((C[0], C[1], C[2], C[3], np.ascontiguousarray(C[4].real))) == 0
    assert plan == L.plan(A, B, form, single_pass=plan["single_pass"])
    return plan


@pytest.mark.parametrize("m", L.ROWS)
def test_every_bin_at_every_row_count(gpu, pkg, O, capfd, switches, truth, m):
    """no switch set: 32-bit keys up to 2^19 (bin X), 2^20 (M) and 2^23 (S) rows and split keys beyond; bin X with the
    heavy columns and the row-range kernel up to 2^21 rows, its own two lists and the dense accumulators beyond"""
    A, B, table, ref = truth(m)
    plan = check_product(pkg, O, capfd, A, B, ref, {})
    # the ladder's products sit in its heavy columns: nothing makes the automatic choice take the ordered form
    assert plan["ordered"] == 0
    assert (plan["xlarge"] + plan["xback"] > 0) == (m > 1 << 21) and plan["medium"] > 0
    assert 0 < plan["dense"] and (plan["dense"] < plan["heavy"]) == (m <= 1 << 21)


@pytest.mark.parametrize("m,form", FORCED, ids=form_id)
def test_forced_forms(gpu, pkg, O, capfd, switches, truth, m, form):
    A, B, table, ref = truth(m)
    switches(form)
    plan = check_product(pkg, O, capfd, A, B, ref, form)
    if form.get("SPL_SPGEMM_TWO_PASS") == "1":
        assert plan["single_pass"] == 0
    if plan["single_pass"] and form.get("SPL_SPGEMM_ORDERED") == "1":
        assert (plan["ordered"], plan["shape"]) == (1, form["SPL_SPGEMM_ORDERED_SHAPE"])
    if form.get("SPL_SPGEMM_X_AS_HEAVY") == "0":
        assert plan["x_heavy"] == 0 and plan["xlarge"] > 0 and plan["xback"] > 0
    if form.get("SPL_SPGEMM_RANGE") == "0":
        assert plan["range"] == 0 and plan["dense"] == plan["heavy"] > 0
    if form.get("SPL_SPGEMM_SPLIT_KEYS") == "1":
        assert plan["key32"] == "0/0/0"


def csc_handle(pkg, m, part=0, nparts=1):
    M = pkg.Matrix(m[1], m[0], m[2], m[3], m[4])
    if np.iscomplexobj(m[4]):
        return pkg.DeviceMatrix.from_csc_complex(M)
    return pkg.DeviceMatrix.from_csc(M, part=part, nparts=nparts)


def test_handle_route(gpu, pkg, O, capfd, switches, truth):
    """device handles hold rows: H(A).spgemm(H(B)) runs the column kernels on B^T A^T, whose "columns of B" are the
    2^21 + 1 rows of A (one to a few hundred products each) and whose row count is the 81 columns of B — whole, and
    with A as the second of three row blocks.  H(B^T).spgemm(H(A^T)) is the ladder itself, 2^21 + 1 rows, on handles."""
    A, B, table, ref = truth(BEYOND)
    At, Bt, Ct = O.transpose(A), O.transpose(B), O.transpose(ref)   # CSR arrays of X = CSC arrays of X^T
    HB = csc_handle(pkg, B)
    (HC, products), plan = planned(capfd, lambda: csc_handle(pkg, A).spgemm(HB))
    rp, ci, v = HC.export_csr()
    assert np.array_equal(rp, Ct[2]) and np.array_equal(ci, Ct[3]) and np.array_equal(v, Ct[4])
    assert products == int(table.products.sum())
    assert plan == L.plan(Bt, At, {}, single_pass=plan["single_pass"]) and plan["rows"] == B[1]
    # rows [r0, r1) of A: block 1 of 3, cut where the entries of A before it reach a third and two thirds
    nnz = int(At[2][-1])
    r0, r1 = (int(np.searchsorted(At[2], (nnz * q) // 3, side="left")) for q in (1, 2))
    assert 0 < r0 < r1 < A[0]
    HA1 = csc_handle(pkg, A, part=1, nparts=3)
    inf = HA1.info()
    assert (inf["row0"], inf["nrows_local"]) == (r0, r1 - r0)
    (HC1, products1), plan1 = planned(capfd, lambda: HA1.spgemm(HB))
    rp1, ci1, v1 = HC1.export_csr()
    a, b = int(Ct[2][r0]), int(Ct[2][r1])
    assert np.array_equal(rp1, Ct[2][r0:r1 + 1] - a) and np.array_equal(ci1, Ct[3][a:b]) and np.array_equal(v1, Ct[4][a:b])
    a, b = int(At[2][r0]), int(At[2][r1])
    At1 = (At[0], r1 - r0, At[2][r0:r1 + 1] - a, At[3][a:b], At[4][a:b])
    assert products1 == int(L.products_and_nb(Bt, At1)[0].sum())
    assert plan1 == L.plan(Bt, At1, {}, single_pass=plan1["single_pass"])
    # the other way round: (A B)^T = B^T A^T on handles is spgemm_device(A, B) itself
    (HCt, productst), plant = planned(capfd, lambda: csc_handle(pkg, Bt).spgemm(csc_handle(pkg, At)))
    rpt, cit, vt = HCt.export_csr()
    assert np.array_equal(rpt, ref[2]) and np.array_equal(cit, ref[3]) and np.array_equal(vt, ref[4])
    assert productst == products
    assert plant == L.plan(A, B, {}, single_pass=plant["single_pass"]) and plant["xback"] > 0


@pytest.mark.parametrize("m", [SMALL, BEYOND])
def test_complex_values(gpu, pkg, O, capfd, switches, truth, m):
    """spl_spgemm_z and two complex handles against O.mm_z: the value kernel works on chunks of 512 entries of a
    column of C and bisects into the columns of A when there are several — columns of 512, 513, 1 024 and 1 025 entries
    and of half a million"""
    A, B, table = L.ladder(m, complex=True)
    ref = O.mm_z(A, B)
    lens = dict(zip(table.names, np.diff(ref[2]).tolist()))
    assert [lens[k] for k in ("c_512", "c_513", "c_1024", "c_1025")] == [512, 513, 1024, 1025]
    assert np.array_equal(ref[3], truth(m)[3][3])   # the pattern of the real ladder
    check_product(pkg, O, capfd, A, B, ref, {})
    (HC, products), plan = planned(capfd, lambda: csc_handle(pkg, A).spgemm(csc_handle(pkg, B)))
    t = K.csr_truth(O, ref)
    rp, ci, v = HC.export_csr()
    assert HC.is_complex and np.array_equal(rp, t.rp) and np.array_equal(ci, t.ci) and np.array_equal(v, t.v)
    assert products == int(table.products.sum())
    assert plan == L.plan(O.transpose(K.real_part(B)), O.transpose(K.real_part(A)), {}, single_pass=plan["single_pass"])


def test_integer_values_against_scipy(gpu, pkg, O, capfd, switches):
    """a second reference that shares no code with the oracle: integer values, every sum exact"""
    A, B, table = L.ladder(BEYOND, values="int")
    C, plan = planned(capfd, lambda: pkg.mm(tuple_to_mat(pkg, A), tuple_to_mat(pkg, B)))
    C = mat_to_tuple(C)
    assert O.check_matrix(C) == 0
    assert L.equals_scipy_product(C, csc_tuple_to_scipy(A) @ csc_tuple_to_scipy(B))
    assert np.array_equal(np.diff(C[2]), np.diff(O.mm(A, B)[2]))   # the sums that cancel stay stored
    assert plan == L.plan(A, B, {}, single_pass=plan["single_pass"])
