"""spl_vector_gram_dev (csrc/gram.hip) and spl_vector_rotate_z_dev (csrc/eigsh.hip) on the device, real and complex.  The
yardstick is the restatement of tests/gram_cases.py (checked on its own in tests/test_gram_cpu.py): every entry of G is
the restated single inner product BIT FOR BIT, whatever the grid, the register tile and the cut into blocks of columns
are, and the rotated columns are the restated ones whatever the tile height is.  All comparisons are by view(uint64)."""
import numpy as np
import pytest

import gram_cases as GK
import krylov_cases as K
from test_gpu_eigsh import SHAPES, device_columns, host_columns, same_with_nan_gaps

pytestmark = pytest.mark.gpu

KNOBS = ("SPL_KRYLOV_GRID", "SPL_GRAM_TILE", "SPL_GRAM_SCRATCH", "SPL_EIGSH_ROTATE_ROWS")
BOTH = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
OK = 0


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the cached inputs are read-only


# ---- 1. the block of inner products ------------------------------------------------------------------------------------------
_gram = {}


def gram_case(n, k, l, cplx):
    """V, W and the restated G of the widest block of this length, computed once; a narrower block is its corner"""
    wide = n <= GK.WIDE_UP_TO
    kmax, lmax = (128, 128) if wide else (5, 127)
    key = (n, cplx)
    if key not in _gram:
        V, W = GK.blocks(n, kmax, lmax, cplx)
        G = GK.gram(V, W)
        for a in (V, W, G):
            a.setflags(write=False)
        _gram[key] = (V, W, G)
    V, W, G = _gram[key]
    assert k <= kmax and l <= lmax
    return V[:, :k], W[:, :l], G[:k, :l]


def raw_gram(pkg, torch, n, k, l, dV, ldv, dW, ldw, ldg, upper, cplx):
    """G as a (ldg x l) array of what the device left in a NaN-filled block"""
    dtype = np.complex128 if cplx else np.float64
    dG = dev(torch, np.full(ldg * l, np.nan, dtype=dtype))
    st = pkg._ffi.lib().spl_vector_gram_dev(n, 2 if cplx else 1, k, l, dV.data_ptr() if n else None, ldv,
                                            dW.data_ptr() if n else None, ldw, dG.data_ptr(), ldg, 1 if upper else 0,
                                            torch.cuda.current_stream().cuda_stream)
    assert st == OK, st
    torch.cuda.synchronize()
    return dG.cpu().numpy().reshape(l, ldg).T


def expected_block(G, ldg, upper):
    """the restated entries where the call writes, NaN everywhere else: below the diagonal with `upper`, and the gap"""
    k, l = G.shape
    out = np.full((ldg, l), np.nan, dtype=G.dtype)
    out[:k, :] = G
    if upper:
        i, j = np.indices((k, l))
        out[:k, :][i > j] = np.nan
    return out


def check_gram(pkg, torch, n, k, l, cplx, pads=(3, 1, 2)):
    V, W, G = gram_case(n, k, l, cplx)
    ldv, ldw, ldg = n + pads[0], n + pads[1], k + pads[2]
    dV, dW = device_columns(torch, V, ldv), device_columns(torch, W, ldw)
    before_v, before_w = dV.cpu().numpy(), dW.cpu().numpy()
    for upper in (False, True):
        got = raw_gram(pkg, torch, n, k, l, dV, ldv, dW, ldw, ldg, upper, cplx)
        want = expected_block(G, ldg, upper)
        assert same_with_nan_gaps(got, want), (n, k, l, cplx, upper)
    assert same_with_nan_gaps(dV.cpu().numpy(), before_v) and same_with_nan_gaps(dW.cpu().numpy(), before_w)


def widths_at(n):
    return [w for w in GK.WIDTHS if n <= GK.WIDE_UP_TO or w not in GK.WIDTHS[-2:]]


@BOTH
@pytest.mark.parametrize("n", GK.LENGTHS)
def test_gram_is_the_restated_dot(gpu, pkg, n, cplx):
    for k, l in widths_at(n):
        check_gram(pkg, gpu, n, k, l, cplx)
    check_gram(pkg, gpu, n, 3, 2, cplx, pads=(0, 0, 0))
    if n == 0:
        got = np.ascontiguousarray(raw_gram(pkg, gpu, 0, 3, 2, None, 0, None, 0, 3, False, cplx))
        assert not np.isnan(got.view(np.float64)).any() and not np.signbit(got.view(np.float64)).any()  # +0.0


def test_gram_middle_level(gpu, pkg):
    """4096^2 + 5 entries: 4097 chunks, so the partials pass a middle level of the fold before the last one"""
    n = 4096 * 4096 + 5
    rng = np.random.default_rng(93)
    w = rng.standard_normal(n)
    V = np.stack([w * np.where((np.arange(n) // 5) % 2 == 0, 1.0, -1.0), rng.standard_normal(n)], axis=1)
    W = np.stack([w, rng.standard_normal(n)], axis=1)
    want = np.array([[K.dot(V[:, i], W[:, j]) for j in range(2)] for i in range(2)])
    dV = gpu.from_numpy(np.ascontiguousarray(V.T).reshape(-1)).cuda()
    dW = gpu.from_numpy(np.ascontiguousarray(W.T).reshape(-1)).cuda()
    got = raw_gram(pkg, gpu, n, 2, 2, dV, n, dW, n, 2, False, False)
    assert K.bits_equal(np.ascontiguousarray(got), want), (got, want)
    assert abs(want[0, 0]) < 1e-3 * n  # it cancels
    # `upper`: the middle level leaves the plane below the diagonal out, and the entry stays what it was
    got = raw_gram(pkg, gpu, n, 2, 2, dV, n, dW, n, 2, True, False)
    assert same_with_nan_gaps(got, expected_block(want, 2, True)), (got, want)


@BOTH
def test_gram_knobs_do_not_show(gpu, pkg, monkeypatch, cplx):
    for grid in ("1", "3", None):
        for tile in GK.TILES + ("7", None):
            for name, value in (("SPL_KRYLOV_GRID", grid), ("SPL_GRAM_TILE", tile)):
                if value is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, value)
            for n, k, l in ((257, 3, 2), (4097, 30, 30), (3 * 4096 + 5, 5, 127), (3 * 4096 + 5, 2, 1)):
                check_gram(pkg, gpu, n, k, l, cplx)


@BOTH
def test_gram_cut_into_blocks_of_columns(gpu, pkg, monkeypatch, cplx):
    """a bound on the partials so small that the call is cut on both sides, down to the smallest block"""
    for scratch in ("1", "4096", "100000"):
        monkeypatch.setenv("SPL_GRAM_SCRATCH", scratch)
        for tile in (None, "1"):
            if tile:
                monkeypatch.setenv("SPL_GRAM_TILE", tile)
            else:
                monkeypatch.delenv("SPL_GRAM_TILE", raising=False)
            for n, k, l in ((4097, 30, 30), (3 * 4096 + 5, 5, 127), (257, 3, 2)):
                check_gram(pkg, gpu, n, k, l, cplx)


@BOTH
def test_gram_against_the_dots_call_column_by_column(gpu, pkg, cplx):
    n, k, l = 3 * 4096 + 5, 5, 127
    V, W, G = gram_case(n, k, l, cplx)
    dV, dW = device_columns(gpu, V, n), device_columns(gpu, W, n)
    got = raw_gram(pkg, gpu, n, k, l, dV, n, dW, n, k, False, cplx)
    out = gpu.full((k,), 7.0, dtype=dV.dtype, device="cuda")
    step = 16 if cplx else 8
    for j in range(l):
        st = pkg._ffi.lib().spl_vector_dots_dev(n, 2 if cplx else 1, k, dV.data_ptr(), n, dW.data_ptr() + j * n * step,
                                                out.data_ptr(), gpu.cuda.current_stream().cuda_stream)
        assert st == OK
        gpu.cuda.synchronize()
        assert K.bits_equal(out.cpu().numpy(), np.ascontiguousarray(got[:, j])), j
    assert K.bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(G))


def test_gram_of_a_block_with_itself_and_the_python_layer(gpu, pkg):
    """the Hermitian use: V == W, the upper triangle, mirrored by the caller"""
    for cplx in (False, True):
        n, k = 4097, 30
        V, _, _ = gram_case(n, k, k, cplx)
        want = GK.gram(V, V)
        dV = device_columns(gpu, V, n + 2)
        G = gpu.full((k * k,), 7.0, dtype=dV.dtype, device="cuda")
        pkg.vector_gram_dev(n, k, k, dV.data_ptr(), n + 2, dV.data_ptr(), n + 2, G.data_ptr(), k, upper=True,
                            is_complex=cplx, stream=gpu.cuda.current_stream().cuda_stream)
        gpu.cuda.synchronize()
        got = G.cpu().numpy().reshape(k, k).T
        i, j = np.indices((k, k))
        assert K.bits_equal(got[i <= j], want[i <= j]) and (got[i > j] == 7.0).all()
        assert (want.diagonal().imag == 0.0).all() if cplx else True


# ---- 2. the rotation with a complex Y --------------------------------------------------------------------------------------
_rotation = {}


def rotation_case(n, m, k):
    key = (n, m, k)
    if key not in _rotation:
        rng = np.random.default_rng(2000 * m + k + n)
        V = rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))
        V[0, 0] = -0.0
        if n > 2:
            V[1, m - 1], V[2, 0] = 5e-324, 1e300
        Y = rng.standard_normal((m, k)) + 1j * rng.standard_normal((m, k))
        Y[m - 1, k - 1] = complex(-0.0, 1.0)
        want = GK.rotate_z(V, Y)
        for a in (V, Y, want):
            a.setflags(write=False)
        _rotation[key] = (V, Y, want)
    return _rotation[key]


def raw_rotate_z(pkg, torch, n, m, k, dV, ldv, dY, ldy, dout, ldo):
    st = pkg._ffi.lib().spl_vector_rotate_z_dev(n, 2, m, k, dV.data_ptr(), ldv, dY.data_ptr(), ldy,
                                                dout.data_ptr() if dout is not None else None, ldo,
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def check_rotation(pkg, torch, n, m, k, ldv, ldy, ldo):
    V, Y, want = rotation_case(n, m, k)
    dY = device_columns(torch, Y, ldy)
    dV = device_columns(torch, V, ldv)
    before = dV.cpu().numpy()
    dout = device_columns(torch, np.full((n, k), 7.0, dtype=V.dtype), ldo)
    assert raw_rotate_z(pkg, torch, n, m, k, dV, ldv, dY, ldy, dout, ldo) == OK
    assert K.bits_equal(host_columns(dout, n, k, ldo), want), (n, m, k, "out")
    assert same_with_nan_gaps(dV.cpu().numpy(), before), "V is untouched"
    expect = device_columns(torch, want, ldo).cpu().numpy()
    assert same_with_nan_gaps(dout.cpu().numpy(), expect), "the rows beyond n are untouched"
    assert raw_rotate_z(pkg, torch, n, m, k, dV, ldv, dY, ldy, None, 0) == OK
    after = before.copy()
    for i in range(k):
        after[i * ldv:i * ldv + n] = want[:, i]
    assert same_with_nan_gaps(dV.cpu().numpy(), after), (n, m, k, "in place: columns k ... and the rows beyond n stay")


@pytest.mark.parametrize("n", [1, 33, 257, 4097, 3 * 4096 + 5])
def test_complex_rotation_is_the_restatement(gpu, pkg, n):
    for m, k in SHAPES:
        check_rotation(pkg, gpu, n, m, k, n + 3, m + 2, n + 1)
    check_rotation(pkg, gpu, n, 3, 2, n, 3, n)


def test_complex_rotation_tile_heights_do_not_show(gpu, pkg, monkeypatch):
    for rows in ("16", "32", "64"):
        monkeypatch.setenv("SPL_EIGSH_ROTATE_ROWS", rows)
        for grid in ("1", None):
            if grid:
                monkeypatch.setenv("SPL_KRYLOV_GRID", grid)
            else:
                monkeypatch.delenv("SPL_KRYLOV_GRID", raising=False)
            for n in (33, 4097):
                for m, k in ((3, 2), (64, 63), (128, 128)):
                    check_rotation(pkg, gpu, n, m, k, n + 3, m + 2, n + 1)


def test_complex_rotation_of_the_python_layer_and_of_nothing(gpu, pkg):
    V, Y, rotated = rotation_case(257, 3, 2)
    dV, dY = device_columns(gpu, V, 260), device_columns(gpu, Y, 3)
    pkg.sparse.vector_rotate_dev(257, 3, 2, dV.data_ptr(), 260, dY.data_ptr(), 3, is_complex=True, Y_is_complex=True)
    gpu.cuda.synchronize()
    assert K.bits_equal(host_columns(dV, 257, 2, 260), rotated)
    before = dV.cpu().numpy()
    assert pkg._ffi.lib().spl_vector_rotate_z_dev(0, 2, 3, 2, None, 0, None, 3, None, 0, None) == OK
    gpu.cuda.synchronize()
    assert same_with_nan_gaps(dV.cpu().numpy(), before)
