"""Aggregation AMG on device handles (spl_matrix_aggregate, spl_amg_*, spl_krylov_set_preconditioner_amg): what the calls
answer before the device is touched, and the yardstick of the GPU tests (tests/amg_cases.py) checked on its own — the
greedy walk against the simulated rounds, the geometry of the aggregates, the payoff in iterations.  What needs a GPU is
in tests/test_gpu_amg.py."""
import ctypes as C

import numpy as np
import pytest

import amg_cases as AK
import coloring_cases as CC
import krylov_cases as K

SYMBOLS = {"spl_matrix_aggregate": 5, "spl_amg_create": 3, "spl_amg_info": 2, "spl_amg_level": 7, "spl_amg_apply_dev": 4,
           "spl_amg_apply": 3, "spl_krylov_set_preconditioner_amg": 2}
CASES = [(name, seed) for name in CC.NAMES for seed in AK.SEEDS]


def _not_a_handle():
    return C.create_string_buffer(256)


def _matrix_magic_only(nrows_global=0, ncols=0, row0=0, nrows_local=0, nnz=0):
    """the magic word of a matrix handle ("SPLM") and its dimensions (magic, device, then nrows_global, ncols, row0,
    nrows_local, nnz as 64-bit words), zeros behind them"""
    buf = C.create_string_buffer(b"MLPS" + bytes(508))
    words = C.cast(buf, C.POINTER(C.c_int64))
    words[1], words[2], words[3], words[4], words[5] = nrows_global, ncols, row0, nrows_local, nnz
    return buf


def _amg_magic_only(n, vw=1):
    """the magic word of an AMG object ("SPLG"), its device, its value width and its size, zeros behind them"""
    buf = C.create_string_buffer(b"GLPS" + bytes(508))
    C.cast(buf, C.POINTER(C.c_int32))[2] = vw
    C.cast(buf, C.POINTER(C.c_int64))[2] = n
    return buf


def _krylov_magic_only(n, vw=1):
    """the magic word of a solver object ("SPLK"), its device, method, value width and size"""
    buf = C.create_string_buffer(b"KLPS" + bytes(508))
    C.cast(buf, C.POINTER(C.c_int32))[3] = vw
    C.cast(buf, C.POINTER(C.c_int64))[2] = n
    return buf


def _aligned(nbytes=64):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, (C.addressof(buf) + 15) & ~15


# ---- the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", CASES)
def test_greedy_and_rounds_agree(name, seed):
    adj = CC.adjacency(CC.pattern(name))
    roots, count = AK.round_roots(adj, seed)
    assert roots == AK.greedy_roots(adj, seed)
    ref = AK.reference(name, seed)
    assert ref.roots.tolist() == roots and ref.rounds == count
    assert (count > 0) == (len(adj) > 0)


@pytest.mark.parametrize("name,seed", CASES)
def test_aggregates_have_the_documented_geometry(name, seed):
    ref = AK.reference(name, seed)
    adj = CC.adjacency(CC.pattern(name))
    roots = ref.roots.tolist()
    root_set = set(roots)
    # roots are pairwise at distance >= 3, and no vertex could be added (maximal)
    for r in roots:
        assert not (AK._within_two(adj, r) & root_set), r
    for v in range(ref.n):
        assert v in root_set or (AK._within_two(adj, v) & root_set), v
    # aggregate k is rooted at the k-th root ascending; every vertex is within distance 2 of its aggregate's root
    assert roots == sorted(roots) and ref.count == len(roots)
    for k, r in enumerate(roots):
        assert ref.agg[r] == k
    for v in range(ref.n):
        r = roots[ref.agg[v]]
        assert v == r or r in AK._within_two(adj, v), v
    if ref.n:
        assert set(ref.agg.tolist()) == set(range(ref.count))
        assert ref.smallest >= 1 and ref.largest <= 1 + ref.max_degree + ref.max_degree * max(ref.max_degree - 1, 0)
    assert 0 <= ref.phase2 <= ref.n - ref.count


def test_the_pinned_cases_of_the_header():
    for seed in AK.SEEDS:
        star = AK.reference("star", seed)
        assert (star.count, star.rounds, star.largest, star.phase2) == (1, 1, 1000, 998)  # vertex 0 is never the first
        diag = AK.reference("diagonal", seed)
        assert diag.count == 50 and diag.agg.tolist() == list(range(50)) and diag.rounds == 1
        assert AK.reference("empty", seed).info() == [0] * 7
        assert AK.reference("one", seed).info() == [1, 1, 1, 1, 1, 0, 0]
        assert np.array_equal(AK.reference("hermitian", seed).agg, AK.reference("poisson", seed).agg)
        assert AK.reference("dense_chain", seed).largest == 70  # the clique is one aggregate
    assert AK.reference("poisson", 0).count == 1177 and AK.reference("poisson", 0).rounds == 5
    assert [L.n for L in AK.cached_hierarchy("poisson", 256)] == [8281, 1177, 75]
    assert [L.n for L in AK.cached_hierarchy("poisson", 16)] == [8281, 1177, 75, 6]
    assert [L.n for L in AK.cached_hierarchy("unsym", 256)] == [300, 2]
    assert [L.n for L in AK.cached_hierarchy("unsymz", 256)] == [300, 3]
    assert [L.n for L in AK.scipy_hierarchy(AK.poisson3d(16))] == [4096, 404, 10]
    assert 1.2 < AK.operator_complexity(AK.cached_hierarchy("poisson", 256)) < 1.5


@pytest.mark.parametrize("method,name", K.CASES)
def test_restated_amg_solve_converges_in_half_the_iterations(method, name):
    out = AK.solve_reference(method, name)
    none = K.reference(method, name, None)
    true = K.true_relative_residual(K.matrix(name), out.x, K.rhs(name))
    print("%s %s: %d iterations with the cycle, %d without, true relative residual %.2e"
          % (method, name, out.iterations, none.iterations, true))
    assert out.reason == 0 and none.reason == 0
    assert 2 * out.iterations <= none.iterations, (out.iterations, none.iterations)
    assert true <= 1e-7, true


def test_the_cycle_is_a_fixed_linear_operator_and_symmetric_for_cg():
    levels = AK.cached_hierarchy("poisson", 256)
    M = AK.Cycle(levels, 1, 4)
    rng = np.random.default_rng(5)
    u, v = rng.uniform(-1, 1, levels[0].n), rng.uniform(-1, 1, levels[0].n)
    Mu, Mv = M(u), M(v)
    assert K.bits_equal(M(u), Mu)
    assert np.linalg.norm(M(u + 2.0 * v) - (Mu + 2.0 * Mv)) <= 1e-12 * np.linalg.norm(Mu + 2.0 * Mv)
    assert abs(np.dot(v, Mu) - np.dot(u, Mv)) <= 1e-12 * np.linalg.norm(v) * np.linalg.norm(Mu)  # <v, M u> = <M v, u>
    assert np.dot(u, Mu) > 0.0


# ---- the surface -------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert L.spl_amg_free.restype is None


def test_the_python_surface_exists(pkg):
    A = pkg.sparse.AMG
    for name in ("info", "level", "apply_dev", "apply", "free"):
        assert callable(getattr(A, name)), name
    assert isinstance(A.levels, property)
    assert pkg.AMG is A and callable(pkg.DeviceMatrix.amg) and callable(pkg.DeviceMatrix.aggregate) and callable(pkg.amg)
    assert len(A.INFO_KEYS) == 8 and len(A.AGGREGATE_KEYS) == 8 and len(A.OPTIONS) == 6
    with pytest.raises(pkg.SparseLinearError):
        pkg.DeviceMatrix(None).amg()
    with pytest.raises(pkg.SparseLinearError):
        pkg.DeviceMatrix(None).aggregate()
    with pytest.raises(TypeError):
        A(pkg.DeviceMatrix(None), cycles=2)


def test_aggregate_refuses_in_the_documented_order(pkg):
    F = pkg._ffi
    L = F.lib()
    keep, at = _aligned()
    info = (C.c_int64 * 8)(*([-7] * 8))
    rect = _matrix_magic_only(3, 2, 0, 3)
    for operand in (None, _not_a_handle()):
        assert L.spl_matrix_aggregate(operand, 0, at, at, info) == F.SPL_ERROR_invalid_handle
        assert L.spl_matrix_aggregate(operand, 0, None, None, None) == F.SPL_ERROR_invalid_handle
    for agg, inf in ((None, info), (at, None), (None, None)):
        assert L.spl_matrix_aggregate(rect, 0, agg, at + 2, inf) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_aggregate(rect, 0, at + 2, at, info) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_aggregate(rect, 0, at, at + 1, info) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_aggregate(rect, 0, at, at, info) == F.SPL_ERROR_dimension_mismatch
    assert L.spl_matrix_aggregate(rect, 7, at, None, info) == F.SPL_ERROR_dimension_mismatch
    block = _matrix_magic_only(4, 4, 2, 2)
    assert L.spl_matrix_aggregate(block, 0, at, at, info) == F.SPL_ERROR_invalid_matrix
    large = _matrix_magic_only(4, 4, 0, 4, 2 ** 31)
    assert L.spl_matrix_aggregate(large, 0, at, at, info) == F.SPL_ERROR_invalid_matrix
    nopointers = _matrix_magic_only(4, 4, 0, 4, 8)  # rows, and no 32-bit row pointers
    assert L.spl_matrix_aggregate(nopointers, 0, at, at, info) == F.SPL_ERROR_invalid_matrix
    assert list(info) == [-7] * 8  # nothing was written by a refusal


def test_amg_create_refuses_in_the_documented_order(pkg):
    F = pkg._ffi
    L = F.lib()
    square = _matrix_magic_only(3, 3, 0, 3)
    rect = _matrix_magic_only(3, 2, 0, 3)

    def options(**kw):
        o = (C.c_int64 * 8)()
        for k, v in kw.items():
            o[int(k[1:])] = v
        return o

    for operand in (None, _not_a_handle()):
        m = C.c_void_p(5)
        assert L.spl_amg_create(operand, None, C.byref(m)) == F.SPL_ERROR_invalid_handle
        assert m.value == 5  # not written: the operand is refused first
    assert L.spl_amg_create(rect, None, None) == F.SPL_ERROR_argument_missing
    bad = [options(o1=5), options(o1=-1), options(o2=-1), options(o3=-2), options(o3=65), options(o4=65), options(o4=-1),
           options(o5=2), options(o5=3), options(o6=1), options(o7=1)]
    for o in bad:
        m = C.c_void_p(5)
        assert L.spl_amg_create(rect, o, C.byref(m)) == F.SPL_ERROR_argument_missing, list(o)
        assert not m.value  # nulled before the options are looked at
    for o in (None, options(), options(o0=-3, o1=4, o2=1, o3=64, o4=64, o5=1)):
        m = C.c_void_p(5)
        assert L.spl_amg_create(rect, o, C.byref(m)) == F.SPL_ERROR_dimension_mismatch and not m.value
    block = _matrix_magic_only(4, 4, 2, 2)
    m = C.c_void_p(5)
    assert L.spl_amg_create(block, None, C.byref(m)) == F.SPL_ERROR_invalid_matrix and not m.value
    nopointers = _matrix_magic_only(4, 4, 0, 4, 8)
    assert L.spl_amg_create(nopointers, None, C.byref(m)) == F.SPL_ERROR_invalid_matrix and not m.value
    assert L.spl_amg_create(square, options(o1=9), C.byref(m)) == F.SPL_ERROR_argument_missing
    info = (C.c_int64 * 8)(*([-7] * 8))
    for operand in (None, _not_a_handle(), square):  # a matrix handle is no AMG object
        assert L.spl_amg_info(operand, info) == F.SPL_ERROR_invalid_handle
        assert L.spl_amg_level(operand, 0, None, None, None, None, None) == F.SPL_ERROR_invalid_handle
    assert list(info) == [-7] * 8
    gone = C.c_void_p()
    L.spl_amg_free(C.byref(gone))  # NULL inside: nothing happens
    L.spl_amg_free(None)


def test_without_a_gpu_the_calls_answer_device(pkg):
    F = pkg._ffi
    if F.device_count() > 0:
        pytest.skip("a GPU is visible")
    keep, at = _aligned()
    info = (C.c_int64 * 8)()
    whole = _matrix_magic_only(0, 0, 0, 0)
    assert F.lib().spl_matrix_aggregate(whole, 0, at, at, info) == F.SPL_ERROR_device
    m = C.c_void_p(5)
    assert F.lib().spl_amg_create(whole, None, C.byref(m)) == F.SPL_ERROR_device and not m.value


def test_amg_apply_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    keep, at = _aligned()
    keep2, other = _aligned()
    for operand in (None, _not_a_handle(), _matrix_magic_only(3, 3, 0, 3)):
        assert L.spl_amg_apply_dev(operand, at, other, None) == F.SPL_ERROR_invalid_handle
        assert L.spl_amg_apply(operand, None, None) == F.SPL_ERROR_invalid_handle
    real, cplx, empty = _amg_magic_only(4), _amg_magic_only(4, 2), _amg_magic_only(0)
    assert L.spl_amg_apply_dev(empty, None, None, None) == F.SPL_OK  # n == 0: nothing is touched
    assert L.spl_amg_apply(empty, None, None) == F.SPL_OK
    for M in (real, cplx):
        assert L.spl_amg_apply_dev(M, None, other, None) == F.SPL_ERROR_argument_missing
        assert L.spl_amg_apply_dev(M, at, None, None) == F.SPL_ERROR_argument_missing
        assert L.spl_amg_apply_dev(M, at, at, None) == F.SPL_ERROR_argument_missing  # in place
        assert L.spl_amg_apply_dev(M, at + 4, other, None) == F.SPL_ERROR_argument_missing
        assert L.spl_amg_apply_dev(M, at, other + 2, None) == F.SPL_ERROR_argument_missing
        assert L.spl_amg_apply(M, None, C.cast(other, F.c_dbl_p)) == F.SPL_ERROR_argument_missing
        assert L.spl_amg_apply(M, C.cast(at, F.c_dbl_p), None) == F.SPL_ERROR_argument_missing
    assert L.spl_amg_apply_dev(cplx, at + 8, other, None) == F.SPL_ERROR_argument_missing  # a pair is 16 bytes
    assert L.spl_amg_apply_dev(cplx, at, other + 8, None) == F.SPL_ERROR_argument_missing


def test_krylov_set_preconditioner_amg_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    solver = _krylov_magic_only(4)
    for operand in (None, _not_a_handle(), _amg_magic_only(4)):
        assert L.spl_krylov_set_preconditioner_amg(operand, _amg_magic_only(4)) == F.SPL_ERROR_invalid_handle
    for M in (_not_a_handle(), _matrix_magic_only(4, 4, 0, 4), _krylov_magic_only(4)):
        assert L.spl_krylov_set_preconditioner_amg(solver, M) == F.SPL_ERROR_invalid_handle
    assert L.spl_krylov_set_preconditioner_amg(solver, _amg_magic_only(5)) == F.SPL_ERROR_dimension_mismatch  # the size
    assert L.spl_krylov_set_preconditioner_amg(solver, _amg_magic_only(4, 2)) == F.SPL_ERROR_dimension_mismatch  # the kind
    assert L.spl_krylov_set_preconditioner_amg(_krylov_magic_only(4, 2), _amg_magic_only(4)) == F.SPL_ERROR_dimension_mismatch
