"""Multicolour ordering on device handles (spl_matrix_color, spl_vector_permute_dev): what the calls answer before the
device is touched, and the yardstick of the GPU tests (tests/coloring_cases.py) checked on its own — the hash against its
pins, the serial colouring against the simulated rounds, the payoff in levels.  What needs a GPU is in
tests/test_gpu_coloring.py."""
import ctypes as C

import numpy as np
import pytest

import coloring_cases as CC

SYMBOLS = {"spl_matrix_color": 7, "spl_vector_permute_dev": 7}
CASES = [(name, seed) for name in CC.NAMES for seed in CC.SEEDS]


def _not_a_handle():
    return C.create_string_buffer(256)


def _matrix_magic_only(nrows_global=0, ncols=0, row0=0, nrows_local=0, nnz=0):
    """the magic word of a matrix handle ("SPLM") and its dimensions (magic, device, then nrows_global, ncols, row0,
    nrows_local, nnz as 64-bit words), zeros behind them"""
    buf = C.create_string_buffer(b"MLPS" + bytes(508))
    words = C.cast(buf, C.POINTER(C.c_int64))
    words[1], words[2], words[3], words[4], words[5] = nrows_global, ncols, row0, nrows_local, nnz
    return buf


def _aligned(nbytes=64):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, (C.addressof(buf) + 15) & ~15


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def test_hash_pins():
    assert CC.priority(0, 0) == 0xe220a8397b1dcdaf
    assert CC.priority(1, 0) == 0x910a2dec89025cc1
    assert CC.priority(2, 0) == 0x975835de1c9756ce
    assert CC.priority(5, 7) == 0x82d78c130699ef2b


@pytest.mark.parametrize("name,seed", CASES)
def test_the_two_restatements_agree(name, seed):
    ref = CC.reference(name, seed)
    colour, count = CC.rounds(CC.adjacency(CC.pattern(name)), seed)
    assert colour == ref.colors.tolist()
    assert count == ref.rounds


@pytest.mark.parametrize("name,seed", CASES)
def test_colourings_are_proper_and_within_the_degree_bound(name, seed):
    ref = CC.reference(name, seed)
    adj = CC.adjacency(CC.pattern(name))
    for v, near in enumerate(adj):
        assert all(ref.colors[u] != ref.colors[v] for u in near), v
    if ref.n:
        assert ref.ncolors <= ref.max_degree + 1
        assert set(ref.colors.tolist()) == set(range(ref.ncolors))  # first fit leaves no colour out
    # the permutation: every vertex once, by colour, ascending inside a class; the offsets are its class boundaries
    assert sorted(ref.perm.tolist()) == list(range(ref.n))
    assert len(ref.offsets) == ref.ncolors + 1 and ref.offsets[0] == 0 and ref.offsets[-1] == ref.n
    for c in range(ref.ncolors):
        members = ref.perm[ref.offsets[c]:ref.offsets[c + 1]]
        assert len(members) > 0 and np.all(ref.colors[members] == c) and np.all(np.diff(members) > 0)


@pytest.mark.parametrize("name,seed", CASES)
def test_levels_of_the_permuted_triangles_are_at_most_the_colours(name, seed):
    ref = CC.reference(name, seed)
    S = CC.permuted(CC.pattern(name), ref.perm) if ref.n else CC.pattern(name)
    assert CC.number_of_levels(S, True) <= ref.ncolors
    assert CC.number_of_levels(S, False) <= ref.ncolors


def test_the_pinned_cases_of_the_header():
    ref = CC.reference("poisson", 0)
    assert (ref.ncolors, ref.rounds) == (5, 12) and np.diff(ref.offsets).tolist() == [3055, 3073, 1577, 564, 12]
    assert CC.number_of_levels(CC.pattern("poisson"), True) == 181
    for seed in CC.SEEDS:
        chain = CC.reference("chain", seed)
        assert chain.ncolors == 3 and CC.number_of_levels(CC.pattern("chain"), True) == 5000
        dense = CC.reference("dense_chain", seed)
        assert (dense.ncolors, dense.rounds) == (70, 70)  # the second window of 64 colours is used
        assert CC.reference("star", seed).max_degree == 999
        assert np.array_equal(CC.reference("hermitian", seed).colors, CC.reference("poisson", seed).colors)
        one = CC.reference("diagonal", seed)
        assert one.ncolors == 1 and one.rounds == 1 and one.perm.tolist() == list(range(50))
        assert CC.reference("empty", seed).offsets.tolist() == [0]
    assert CC.reference("unsym", 0).max_degree == 65
    # every edge of `upper` is stored on one side: the transposed pattern is needed to see the lower neighbours
    U = CC.pattern("upper")
    assert U.nnz > 0 and (U.indices >= np.repeat(np.arange(200), np.diff(U.indptr)) + 1).all()
    Z = CC.pattern("zeros")
    assert (Z.data == 0.0).sum() == Z.nnz - 150 and CC.reference("zeros", 0).ncolors > 1


def test_restated_multicolour_ilu0_converges_and_beats_no_preconditioner():
    """CG on the 91 x 91 Laplacian in the multicolour numbering: more iterations than natural ILU(0), fewer than none"""
    import krylov_cases as K
    S, b = K.matrix("poisson"), K.rhs("poisson")
    x, pre = CC.cached_solve_reference("cg", "poisson", "ilu0")
    _, none = CC.cached_solve_reference("cg", "poisson", None)
    assert pre.reason == 0 and none.reason == 0
    assert K.true_relative_residual(S, x, b) <= 10 * K.RTOL
    assert K.reference("cg", "poisson", "ilu0").iterations <= pre.iterations < none.iterations
    assert none.iterations == K.reference("cg", "poisson", None).iterations  # a permutation of CG without M: same count


# ---- the surface -------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported(pkg):
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert pkg._ffi.SPL_COLOR_hash == 0


def test_the_python_surface_exists(pkg):
    K = pkg.sparse.Coloring
    for name in ("info", "permute", "to_permuted", "from_permuted", "krylov"):
        assert callable(getattr(K, name)), name
    assert pkg.Coloring is K and callable(pkg.DeviceMatrix.coloring) and callable(pkg.multicolor)
    assert pkg.multicolor is pkg.sparse.multicolor and callable(pkg.vector_permute_dev)
    assert len(K.INFO_KEYS) == 8 and len(set(K.INFO_KEYS)) == 8
    for name in ("solve", "info", "free"):
        assert callable(getattr(pkg.sparse.MulticolorKrylov, name)), name
    with pytest.raises(pkg.SparseLinearError):
        pkg.DeviceMatrix(None).coloring()


def test_color_refuses_in_the_documented_order(pkg):
    F = pkg._ffi
    L = F.lib()
    keep, at = _aligned()
    info = (C.c_int64 * 8)(*([-7] * 8))
    rect = _matrix_magic_only(3, 2, 0, 3)
    # 1. the handle, before anything is written
    for operand in (None, _not_a_handle()):
        off = F.c_i64_p(C.c_int64(5))
        assert L.spl_matrix_color(operand, 0, 0, at, at, C.byref(off), info) == F.SPL_ERROR_invalid_handle
        assert bool(off)  # not written: the operand is refused first
        assert L.spl_matrix_color(operand, 9, 0, None, None, None, None) == F.SPL_ERROR_invalid_handle
    # 2. d_colors or info missing; *offsets is nulled first
    for colors, inf in ((None, info), (at, None), (None, None)):
        off = F.c_i64_p(C.c_int64(5))
        assert L.spl_matrix_color(rect, 9, 0, colors, at + 2, C.byref(off), inf) == F.SPL_ERROR_argument_missing
        assert not off
    # 3. an unknown order, an unaligned array: before the shape is looked at
    assert L.spl_matrix_color(rect, 1, 0, at, at, None, info) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_color(rect, -1, 0, at, None, None, info) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_color(rect, 0, 0, at + 2, at, None, info) == F.SPL_ERROR_argument_missing
    assert L.spl_matrix_color(rect, 0, 0, at, at + 1, None, info) == F.SPL_ERROR_argument_missing
    # 4. not square
    assert L.spl_matrix_color(rect, 0, 0, at, at, None, info) == F.SPL_ERROR_dimension_mismatch
    assert L.spl_matrix_color(rect, 0, 0, at, None, None, info) == F.SPL_ERROR_dimension_mismatch
    # 5. a row block, or 2^31 entries and more
    block = _matrix_magic_only(4, 4, 2, 2)  # rows 2, 3 of a 4 x 4 matrix
    assert L.spl_matrix_color(block, 0, 0, at, at, None, info) == F.SPL_ERROR_invalid_matrix
    large = _matrix_magic_only(4, 4, 0, 4, 2 ** 31)
    assert L.spl_matrix_color(large, 0, 7, at, at, None, info) == F.SPL_ERROR_invalid_matrix
    assert list(info) == [-7] * 8  # nothing was written by a refusal


def test_without_a_gpu_color_answers_device(pkg):
    F = pkg._ffi
    if F.device_count() > 0:
        pytest.skip("a GPU is visible")
    keep, at = _aligned()
    info = (C.c_int64 * 8)()
    off = F.c_i64_p(C.c_int64(5))
    whole = _matrix_magic_only(0, 0, 0, 0)
    assert F.lib().spl_matrix_color(whole, 0, 0, at, at, C.byref(off), info) == F.SPL_ERROR_device and not off


def test_vector_permute_refuses_before_the_device(pkg):
    F = pkg._ffi
    L = F.lib()
    keep, at = _aligned()
    keep2, other = _aligned()
    assert L.spl_vector_permute_dev(-1, 1, at, 0, at, other, None) == F.SPL_ERROR_n_nonpositive
    for width in (0, 3):
        assert L.spl_vector_permute_dev(4, width, at, 0, at, other, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_permute_dev(4, 1, None, 0, at, other, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_permute_dev(4, 1, at, 0, None, other, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_permute_dev(4, 1, at, 1, at, None, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_permute_dev(4, 1, at, 0, other, other, None) == F.SPL_ERROR_argument_missing  # in place
    assert L.spl_vector_permute_dev(4, 1, at + 2, 0, at, other, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_permute_dev(4, 1, at, 0, at + 4, other, None) == F.SPL_ERROR_argument_missing
    assert L.spl_vector_permute_dev(4, 2, at, 0, at + 8, other, None) == F.SPL_ERROR_argument_missing  # a pair is 16 bytes
    assert L.spl_vector_permute_dev(4, 2, at, 1, at, other + 8, None) == F.SPL_ERROR_argument_missing
