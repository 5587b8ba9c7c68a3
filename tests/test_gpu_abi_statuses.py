"""The C ABI's error contract, called raw through ctypes: the status every entry point returns for a malformed
input, and the NULL it leaves in its output pointers.  The Python layer validates first and never reaches most of
these paths.  Plus one success case per value width with unsorted input columns, which must give bit for bit what
the same matrix with sorted columns gives."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK = 0
ARG = -5          # SPL_ERROR_argument_missing
NEG = -6          # SPL_ERROR_n_nonpositive
INVALID = -8      # SPL_ERROR_invalid_matrix
DIM = -20         # SPL_ERROR_dimension_mismatch
OOB = -21         # SPL_ERROR_index_out_of_bounds
OVERFLOW = -22    # SPL_ERROR_index_overflow

ip = C.POINTER(C.c_int)
vp = C.c_void_p


def ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def dbls(*v):
    return (C.c_double * max(len(v), 1))(*v)


# 3 x 3 CSC with ascending rows in every column; UNSORTED is the same matrix with columns 0 and 2 reversed
AP = (0, 2, 3, 5)
AI = (0, 2, 1, 0, 2)
AX = (1.5, -2.0, 3.25, 0.5, 4.0)
AI_UNSORTED = (2, 0, 1, 2, 0)
AX_UNSORTED = (-2.0, 1.5, 3.25, 4.0, 0.5)
AZ = (1.5, 0.25, -2.0, 1.0, 3.25, -0.5, 0.5, 2.0, 4.0, -1.0)
AZ_UNSORTED = (-2.0, 1.0, 1.5, 0.25, 3.25, -0.5, 4.0, -1.0, 0.5, 2.0)


def tup(nrows=3, ncols=3, p=AP, i=AI, x=AX):
    """a CSC 5-tuple as ctypes arguments; None leaves a pointer NULL"""
    return (nrows, ncols, ints(*p) if p is not None else None, ints(*i) if i is not None else None,
            dbls(*x) if x is not None else None)


BAD_TUPLES = [
    # (label, tuple, status)
    ("negative nrows", tup(nrows=-1), NEG),
    ("negative ncols", tup(ncols=-1, p=(0,)), NEG),
    ("NULL Ap", tup(p=None), ARG),
    ("NULL Ai", tup(i=None), ARG),
    ("NULL Ax", tup(x=None), ARG),
    ("non-monotone Ap", tup(p=(0, 3, 2, 5)), INVALID),
    ("row out of range", tup(i=(0, 3, 1, 0, 2)), INVALID),
]
BAD_TUPLES_Z = [(lbl, t[:4] + ((dbls(*AZ) if t[4] is not None else None),), st) for lbl, t, st in BAD_TUPLES]
BAD_IDS = [b[0] for b in BAD_TUPLES]


@pytest.fixture(scope="module")
def L(pkg, gpu):
    return pkg._ffi.lib()


def new_handle(L, t=None):
    h = vp()
    assert L.spl_matrix_create(*(t or tup()), C.byref(h)) == OK
    return h


def free_handle(L, h):
    L.spl_matrix_free(C.byref(h))


def take(L, ptr, n, ctype, dtype):
    arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).astype(dtype, copy=True)
    L.spl_free(ptr)
    return arr


# ---- handles -------------------------------------------------------------------------------------------------


def test_create_rowblock_null_output(L):
    assert L.spl_matrix_create_rowblock(*tup(), 0, 1, None) == ARG


@pytest.mark.parametrize("label,t,status", BAD_TUPLES, ids=BAD_IDS)
def test_create_rowblock_bad_tuple(L, label, t, status):
    h = vp(1)
    assert L.spl_matrix_create_rowblock(*t, 0, 1, C.byref(h)) == status
    assert not h.value


@pytest.mark.parametrize("part,nparts", [(-1, 2), (2, 2), (0, 0), (0, -1)])
def test_create_rowblock_bad_part(L, part, nparts):
    h = vp(1)
    assert L.spl_matrix_create_rowblock(*tup(), part, nparts, C.byref(h)) == ARG
    assert not h.value


def test_create_z_null_output(L):
    assert L.spl_matrix_create_z(*tup(x=AZ), None) == ARG


@pytest.mark.parametrize("label,t,status", BAD_TUPLES_Z, ids=BAD_IDS)
def test_create_z_bad_tuple(L, label, t, status):
    h = vp(1)
    assert L.spl_matrix_create_z(*t, C.byref(h)) == status
    assert not h.value


def test_create_csr_statuses(L):
    rp, ci, v = ints(*AP), ints(*AI), dbls(*AX)
    assert L.spl_matrix_create_csr(3, 3, 0, 3, rp, ci, v, None) == ARG
    cases = [
        ((-1, 3, 0, 3, rp, ci, v), NEG),
        ((3, -1, 0, 3, rp, ci, v), NEG),
        ((3, 3, -1, 3, rp, ci, v), NEG),
        ((3, 3, 1, 3, rp, ci, v), ARG),            # row0 + nrows_local > nrows_global
        ((3, 3, 0, 3, None, ci, v), ARG),
        ((3, 3, 0, 3, ints(0, 1, 1, -1), ci, v), INVALID),
        ((3, 3, 0, 3, rp, None, v), ARG),
        ((3, 3, 0, 3, rp, ci, None), ARG),
        ((3, 3, 0, 3, ints(0, 3, 2, 5), ci, v), INVALID),
        ((3, 2, 0, 3, rp, ci, v), INVALID),        # column 2 out of range
    ]
    for args, status in cases:
        h = vp(1)
        assert L.spl_matrix_create_csr(*args, C.byref(h)) == status, args
        assert not h.value


def test_create_synthetic_and_rmat_statuses(L):
    assert L.spl_matrix_create_synthetic(0, 100, 4, 1, 0, 100, None) == ARG
    assert L.spl_matrix_create_rmat(4, 4, 0.5, 0.2, 0.2, 1, None) == ARG
    for args, status in [((4, 100, 4, 1, 0, 100), ARG), ((0, 100, 0, 1, 0, 100), ARG), ((3, 2000, 4, 1, 0, 10), OVERFLOW),
                         ((1, 100, 4, 1, 50, 10), ARG)]:
        h = vp(1)
        assert L.spl_matrix_create_synthetic(*args, C.byref(h)) == status, args
        assert not h.value
    for args, status in [((0, 4, 0.5, 0.2, 0.2, 1), ARG), ((4, 4, 0.6, 0.3, 0.3, 1), ARG), ((30, 4, 0.5, 0.2, 0.2, 1), OVERFLOW)]:
        h = vp(1)
        assert L.spl_matrix_create_rmat(*args, C.byref(h)) == status, args
        assert not h.value


def test_matrix_spgemm_statuses(L):
    A = new_handle(L)
    B = new_handle(L, tup(nrows=2, ncols=3, i=(0, 1, 1, 0, 1)))  # 2 x 3: A * B mismatches
    try:
        assert L.spl_matrix_spgemm(A, A, None, None) == ARG
        hc = vp(1)
        assert L.spl_matrix_spgemm(A, B, C.byref(hc), None) == DIM
        assert not hc.value
        assert L.spl_matrix_spgemm(A, None, C.byref(hc), None) == -3  # SPL_ERROR_invalid_handle
    finally:
        free_handle(L, A)
        free_handle(L, B)


def test_create_z_unsorted_columns_bitwise(L):
    images = []
    for i, z in ((AI, AZ), (AI_UNSORTED, AZ_UNSORTED)):
        h = vp()
        assert L.spl_matrix_create_z(*tup(i=i, x=z), C.byref(h)) == OK
        rp, ci, v = (C.c_int64 * 4)(), (C.c_int * 5)(), (C.c_double * 10)()
        try:
            assert L.spl_matrix_export_csr(h, rp, ci, v) == OK
        finally:
            free_handle(L, h)
        images.append((list(rp), list(ci), np.array(v[:]).view(np.uint64).tolist()))
    assert images[0] == images[1]
    assert images[0][0] == [0, 2, 3, 5]


# ---- one-shot SpMV / SpMM ------------------------------------------------------------------------------------


@pytest.mark.parametrize("label,t,status", BAD_TUPLES, ids=BAD_IDS)
def test_gaxpy_mulv_mulm_bad_tuple(L, label, t, status):
    nrows, ncols = max(t[0], 0), max(t[1], 0)
    x, y = dbls(*([1.0] * 3)), dbls(*([0.0] * 3))
    assert L.spl_gaxpy(*t, ncols, x, nrows, y) == status
    assert L.spl_mulv(*t, ncols, x, y) == status
    assert L.spl_mulm(*t, ncols, 1, x, y) == status


def test_gaxpy_mulv_mulm_shape(L):
    x, y = dbls(1.0, 1.0, 1.0, 1.0), dbls(0.0, 0.0, 0.0, 0.0)
    assert L.spl_gaxpy(*tup(), 2, x, 3, y) == DIM
    assert L.spl_gaxpy(*tup(), 3, x, 4, y) == DIM
    assert L.spl_mulv(*tup(), 4, x, y) == DIM
    assert L.spl_mulm(*tup(), 2, 1, x, y) == DIM
    assert L.spl_mulm(*tup(), 3, -1, x, y) == NEG
    assert L.spl_mulm(*tup(), 3, 1, None, y) == ARG
    assert L.spl_mulm(*tup(), 3, 1, x, None) == ARG
    assert L.spl_mulv(*tup(), 3, None, y) == ARG


# ---- binary one-shots ----------------------------------------------------------------------------------------


def binary(L, name, a, b, nrc=True, ncc=True, outs=(True, True, True), alpha=None, beta=None):
    """call a binary one-shot; returns (status, (Cp, Ci, Cx) values, (nrowsC, ncolsC))"""
    nr, nc = C.c_int(-7), C.c_int(-7)
    cp, ci, cx = vp(1), vp(1), vp(1)
    o = [C.byref(p) if want else None for p, want in zip((cp, ci, cx), outs)]
    tail = [C.byref(nr) if nrc else None, C.byref(nc) if ncc else None] + o
    fn = getattr(L, name)
    if name == "spl_lin":
        st = fn(1.25 if alpha is None else alpha, *a, -0.75 if beta is None else beta, *b, *tail)
    elif name == "spl_lin_z":
        st = fn(dbls(1.25, 0.5) if alpha is None else alpha, *a, dbls(-0.75, 2.0) if beta is None else beta, *b, *tail)
    else:
        st = fn(*a, *b, *tail)
    return st, (cp, ci, cx), (nr.value, nc.value)


def free_outputs(L, ptrs):
    for p in ptrs:
        if p.value:
            L.spl_free(p)


BINARY = ["spl_spgemm", "spl_lin", "spl_kronecker", "spl_spgemm_z", "spl_lin_z"]


def operands(name):
    return (tup(x=AZ), tup(x=AZ)) if name.endswith("_z") else (tup(), tup())


@pytest.mark.parametrize("name", BINARY)
def test_binary_null_outputs(L, name):
    a, b = operands(name)
    for kw in (dict(nrc=False), dict(ncc=False), dict(outs=(False, True, True)), dict(outs=(True, False, True)),
               dict(outs=(True, True, False))):
        st, ptrs, _ = binary(L, name, a, b, **kw)
        assert st == ARG, kw
        # refused before anything is written: the outputs that were passed keep what they held
        assert all(p.value == 1 for p, want in zip(ptrs, kw.get("outs", (True, True, True))) if want), kw


@pytest.mark.parametrize("name", BINARY)
@pytest.mark.parametrize("label,t,status", BAD_TUPLES, ids=BAD_IDS)
@pytest.mark.parametrize("side", ["A", "B"])
def test_binary_bad_tuple(L, name, label, t, status, side):
    bad = BAD_TUPLES_Z[BAD_IDS.index(label)][1] if name.endswith("_z") else t
    good = operands(name)[0]
    a, b = (bad, good) if side == "A" else (good, bad)
    st, ptrs, _ = binary(L, name, a, b)
    assert st == status
    assert all(not p.value for p in ptrs)


@pytest.mark.parametrize("name", ["spl_spgemm", "spl_spgemm_z", "spl_lin", "spl_lin_z"])
def test_binary_shape_mismatch(L, name):
    z = name.endswith("_z")
    a = tup(x=AZ) if z else tup()
    b = tup(nrows=2, ncols=3, i=(0, 1, 1, 0, 1), x=AZ if z else AX)  # 2 x 3
    st, ptrs, _ = binary(L, name, a, b)
    assert st == DIM
    assert all(not p.value for p in ptrs)


def test_lin_z_null_scalars(L):
    a, b = tup(x=AZ), tup(x=AZ)
    for alpha, beta in ((None, dbls(1.0, 0.0)), (dbls(1.0, 0.0), None)):
        nr, nc, cp, ci, cx = C.c_int(), C.c_int(), vp(1), vp(1), vp(1)
        st = L.spl_lin_z(alpha, *a, beta, *b, C.byref(nr), C.byref(nc), C.byref(cp), C.byref(ci), C.byref(cx))
        assert st == ARG
        # the scalars are checked with the output pointers, before the outputs are cleared
        assert cp.value == 1 and ci.value == 1 and cx.value == 1


def test_kronecker_statuses(L):
    st, ptrs, _ = binary(L, "spl_kronecker", tup(), tup(nrows=-2, ncols=3))
    assert st == NEG and all(not p.value for p in ptrs)
    big = (50000, 1, ints(0, 0), None, None)
    st, ptrs, _ = binary(L, "spl_kronecker", big, big)
    assert st == OVERFLOW and all(not p.value for p in ptrs)
    wide = (1, 50000, ints(*([0] * 50001)), None, None)
    st, ptrs, _ = binary(L, "spl_kronecker", wide, wide)
    assert st == OVERFLOW and all(not p.value for p in ptrs)


@pytest.mark.parametrize("name", ["spl_spgemm", "spl_lin", "spl_spgemm_z", "spl_lin_z"])
def test_binary_unsorted_columns_bitwise(L, name):
    z = name.endswith("_z")
    sorted_t = tup(x=AZ) if z else tup()
    unsorted_t = tup(i=AI_UNSORTED, x=AZ_UNSORTED if z else AX_UNSORTED)
    results = []
    for a, b in ((sorted_t, sorted_t), (unsorted_t, unsorted_t)):
        st, (cp, ci, cx), shape = binary(L, name, a, b)
        assert st == OK and shape == (3, 3)
        p = take(L, cp, 4, C.c_int, np.int32)
        nz = int(p[-1])
        i = take(L, ci, max(nz, 1), C.c_int, np.int32)[:nz]
        x = take(L, cx, max(nz, 1) * (2 if z else 1), C.c_double, np.float64)[:nz * (2 if z else 1)]
        results.append((p.tolist(), i.tolist(), x.view(np.uint64).tolist()))
    assert results[0] == results[1]
    assert results[0][0][-1] > 0


# ---- assembly and compress -----------------------------------------------------------------------------------


def assemble(L, blocks, value_width=1, row_off=(0,), col_off=(0,), nrowsC=3, ncolsC=3, outs=(True, True, True)):
    k = len(blocks)
    nr = ints(*[b[0] for b in blocks])
    nc = ints(*[b[1] for b in blocks])
    ap = (vp * max(k, 1))(*[C.cast(b[2], vp) if b[2] is not None else None for b in blocks])
    ai = (vp * max(k, 1))(*[C.cast(b[3], vp) if b[3] is not None else None for b in blocks])
    ax = (vp * max(k, 1))(*[C.cast(b[4], vp) if b[4] is not None else None for b in blocks])
    cp, ci, cx = vp(1), vp(1), vp(1)
    o = [C.byref(p) if want else None for p, want in zip((cp, ci, cx), outs)]
    fn = L.spl_assemble_blocks
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, ip, ip, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int, ip, ip, C.c_int, C.c_int,
                   C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    st = fn(k, nr, nc, ap, ai, ax, value_width, ints(*row_off), ints(*col_off), nrowsC, ncolsC, *o)
    return st, (cp, ci, cx)


def test_assemble_blocks_statuses(L):
    for outs in ((False, True, True), (True, False, True), (True, True, False)):
        st, ptrs = assemble(L, [tup()], outs=outs)
        assert st == ARG
        assert all(p.value == 1 for p, want in zip(ptrs, outs) if want)
    cases = [
        (dict(blocks=[tup()], value_width=3), ARG),
        (dict(blocks=[tup()], nrowsC=-1), ARG),
        (dict(blocks=[tup()], row_off=(1,)), DIM),           # block overhangs the result
        (dict(blocks=[tup()], col_off=(-1,)), DIM),
        (dict(blocks=[tup(nrows=-1)]), DIM),
        (dict(blocks=[tup(p=None)]), ARG),
        (dict(blocks=[tup(p=(0, 1, 1, -1))]), ARG),            # Ap[b][ncols] < 0
        (dict(blocks=[tup(i=None)]), ARG),
        (dict(blocks=[tup(p=(0, 3, 2, 5))]), INVALID),
        (dict(blocks=[tup(i=(0, 3, 1, 0, 2))]), INVALID),
    ]
    for kw, status in cases:
        st, ptrs = assemble(L, **kw)
        assert st == status, kw
        assert all(not p.value for p in ptrs), kw


def test_compress_statuses(L):
    rows, cols, vals = ints(0, 1, 2), ints(0, 1, 2), dbls(1.0, 2.0, 3.0)
    Ap = ints(0, 0, 0, 0)
    ai, ax = vp(1), vp(1)
    assert L.spl_compress(3, 3, 3, rows, cols, vals, None, C.byref(ai), C.byref(ax), None) == ARG
    assert L.spl_compress(3, 3, 3, rows, cols, vals, Ap, None, C.byref(ax), None) == ARG
    assert L.spl_compress(3, 3, 3, rows, cols, vals, Ap, C.byref(ai), None, None) == ARG
    assert ai.value == 1 and ax.value == 1  # refused before anything is written
    bad = C.c_int64(-9)
    cases = [
        ((-1, 3, 3, rows, cols, vals), NEG, -9),
        ((3, 3, -1, rows, cols, vals), NEG, -9),
        ((3, 3, 0x7fffffff, rows, cols, vals), OVERFLOW, -9),
        ((3, 3, 3, None, cols, vals), ARG, -9),
        ((3, 3, 3, rows, cols, None), ARG, -9),
        ((3, 3, 3, ints(0, 3, 1), cols, vals), OOB, 1),         # row 3 at position 1
        ((3, 3, 3, rows, ints(0, 1, -1), vals), OOB, 2),        # column -1 at position 2
        ((3, 3, 3, ints(0, 1, 5), ints(0, -1, 2), vals), OOB, 2),  # rows are checked before columns
    ]
    for args, status, where in cases:
        ai, ax = vp(1), vp(1)
        bad.value = -9
        assert L.spl_compress(*args, Ap, C.byref(ai), C.byref(ax), C.byref(bad)) == status, args
        assert not ai.value and not ax.value
        assert bad.value == where, args
