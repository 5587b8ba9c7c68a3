"""Multicolour ordering on device handles (csrc/coloring.hip): spl_matrix_color, spl_vector_permute_dev and the Python
layer on them.  The yardstick is the restatement of tests/coloring_cases.py (checked on its own in
tests/test_coloring_cpu.py): the device's colours, permutation, offsets, colour count and round count must equal it
EXACTLY, whatever the grid and the host's check interval are; the solves in the new numbering must equal the restated
drivers of tests/krylov_cases.py bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import coloring_cases as CC
import krylov_cases as K

pytestmark = pytest.mark.gpu

KNOBS = ("SPL_COLOR_CHECK_EVERY", "SPL_COLOR_GRID", "SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS", "SPL_KRYLOV_GRID")
CASES = [(name, seed) for name in CC.NAMES for seed in CC.SEEDS]


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def handle_of(pkg, S):
    """a whole device handle with the entries of the scipy matrix S (explicit zeros included), real or complex"""
    if S.shape[0] == 0:
        return pkg.DeviceMatrix.ident(0)
    S = sp.csc_matrix(S)
    S.sort_indices()
    M = pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)
    return pkg.DeviceMatrix.from_csc_complex(M) if np.iscomplexobj(S.data) else pkg.DeviceMatrix.from_csc(M)


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def raw_color(pkg, torch, H, n, seed, with_perm=True, with_offsets=True):
    """spl_matrix_color through ctypes: (colors, perm or None, offsets or None, info)"""
    F = pkg._ffi
    colors = torch.full((max(n, 1),), -5, dtype=torch.int32, device="cuda")
    perm = torch.full((max(n, 1),), -5, dtype=torch.int32, device="cuda")
    info = (C.c_int64 * 8)(*([-7] * 8))
    off = F.c_i64_p()
    torch.cuda.synchronize()
    st = F.lib().spl_matrix_color(H.handle, 0, seed, colors.data_ptr(), perm.data_ptr() if with_perm else None,
                                  C.byref(off) if with_offsets else None, info)
    assert st == 0, st
    info = list(info)
    offsets = F.take_malloced(off, info[1] + 1, C.c_int64, np.int64) if with_offsets else None
    return colors.cpu().numpy()[:n], perm.cpu().numpy()[:n] if with_perm else None, offsets, info


def assert_is_the_reference(got, ref, what=""):
    colors, perm, offsets, info = got
    assert np.array_equal(colors, ref.colors), (what, "colors", int(np.argmax(colors != ref.colors)) if ref.n else None)
    assert info[0] == ref.n and info[1] == ref.ncolors and info[2] == ref.rounds, (what, info, ref.ncolors, ref.rounds)
    if perm is not None:
        assert perm.dtype == np.int32 and np.array_equal(perm, ref.perm), (what, "perm")
    if offsets is not None:
        assert offsets.dtype == np.int64 and np.array_equal(offsets, ref.offsets), (what, offsets, ref.offsets)
    sizes = np.diff(ref.offsets)
    assert info[3] == (int(sizes.max()) if ref.n else 0) and info[4] == (int(sizes.min()) if ref.n else 0), (what, info)
    assert info[5] == ref.max_degree and info[7] == 0, (what, info)
    assert (info[6] > ref.rounds) if ref.n else info[6] == 0, (what, info)


# ---- 1. exactness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", CASES)
def test_colours_permutation_offsets_and_rounds_are_the_restatement(gpu, pkg, name, seed):
    ref = CC.reference(name, seed)
    H = handle_of(pkg, CC.pattern(name))
    assert H.is_complex == (name == "hermitian")
    assert_is_the_reference(raw_color(pkg, gpu, H, ref.n, seed), ref, (name, seed))
    # d_perm and offsets are optional: the colours do not depend on them
    assert_is_the_reference(raw_color(pkg, gpu, H, ref.n, seed, with_perm=False, with_offsets=False), ref, "bare")
    H.free()


def test_the_pinned_laplacian(gpu, pkg):
    """seed 0 on the 91 x 91 Laplacian: 5 colours of 3055, 3073, 1577, 564 and 12 vertices in 12 rounds; the complex
    handle of the Hermitian case gives the real pattern's arrays"""
    real = raw_color(pkg, gpu, handle_of(pkg, CC.pattern("poisson")), 8281, 0)
    assert real[3][1] == 5 and real[3][2] == 12 and np.diff(real[2]).tolist() == [3055, 3073, 1577, 564, 12]
    cplx = raw_color(pkg, gpu, handle_of(pkg, CC.pattern("hermitian")), 8281, 0)
    assert np.array_equal(real[0], cplx[0]) and np.array_equal(real[1], cplx[1]) and np.array_equal(real[2], cplx[2])
    assert real[3][:6] == cplx[3][:6]


# ---- 2. launch shapes do not show --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson", "dense_chain", "unsym", "star"])
def test_check_interval_and_grid_do_not_show(gpu, pkg, monkeypatch, name):
    seed = 7
    ref = CC.reference(name, seed)
    H = handle_of(pkg, CC.pattern(name))
    launches = {}
    for every in ("1", "64"):
        for grid in ("1", "65536"):
            monkeypatch.setenv("SPL_COLOR_CHECK_EVERY", every)
            monkeypatch.setenv("SPL_COLOR_GRID", grid)  # one workgroup walks every worklist, ..., the default cap
            got = raw_color(pkg, gpu, H, ref.n, seed)
            assert_is_the_reference(got, ref, (name, every, grid))
            launches[(every, grid)] = got[3][6]
    # the knob was read: rounds are issued in batches of 64, the last ones on an empty worklist
    extra = launches[("1", "1")] - ref.rounds
    assert launches[("1", "65536")] == launches[("1", "1")] and extra > 0
    assert launches[("64", "1")] == extra + 64 * -(-ref.rounds // 64)
    H.free()


# ---- 3. the payoff: levels of the solves and of ILU(0) -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson", "chain", "unsym", "dense_chain", "star"])
def test_levels_are_at_most_the_colours(gpu, pkg, name):
    ref = CC.reference(name, 0)
    H = handle_of(pkg, CC.pattern(name))
    col = H.coloring(0)
    assert col.ncolors == ref.ncolors
    B = col.permute()
    lower, upper, ilu = B.triangular("lower"), B.triangular("upper"), pkg.ILU0(B)
    levels = (lower.info()["levels"], upper.info()["levels"], ilu.info()["levels"], ilu.lower.info()["levels"],
              ilu.upper.info()["levels"])
    print("%s: %d colours, levels of tril / triu / ILU(0) / its L / its U in the new numbering: %s" % (name, ref.ncolors, levels))
    assert all(0 < v <= ref.ncolors for v in levels), (levels, ref.ncolors)
    if name == "chain":
        natural = H.ilu0()
        assert natural.info()["levels"] == 5000 and max(levels) <= 3
        natural.free()
    # P A P^T is the matrix the restatement permutes
    rp, ci, v = B.export_csr()
    want = CC.permuted(CC.pattern(name), ref.perm)
    assert np.array_equal(rp, want.indptr) and np.array_equal(ci, want.indices) and np.array_equal(v, want.data)
    for part in (lower, upper, ilu, B, H):
        part.free()


# ---- 4. spl_vector_permute_dev ------------------------------------------------------------------------------------------
def special_values(n, cplx, seed):
    """values whose bits matter: NaNs with payloads, -0.0, infinities and subnormals among ordinary numbers"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 63, n * (2 if cplx else 1), dtype=np.uint64) | \
        (rng.integers(0, 2, n * (2 if cplx else 1), dtype=np.uint64) << np.uint64(63))
    odd = np.array([0x8000000000000000, 0x7FF8000000000123, 0xFFF0000000000001, 0x7FF0000000000000, 0x0000000000000001,
                    0xFFF8DEADBEEF0001], dtype=np.uint64)
    bits[:min(len(odd), len(bits))] = odd[:len(bits)]
    v = bits.view(np.float64)
    return v.view(np.complex128) if cplx else v


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", ["poisson", "unsym", "one", "empty"])
def test_vector_permute_moves_bits(gpu, pkg, name, cplx):
    ref = CC.reference(name, 7)
    n = ref.n
    perm = dev(gpu, ref.perm) if n else gpu.zeros(0, dtype=gpu.int32, device="cuda")
    v = special_values(n, cplx, 17 + n)
    dv = dev(gpu, v)
    L = pkg._ffi.lib()
    stream = gpu.cuda.current_stream().cuda_stream
    words = 2 if cplx else 1
    fwd = gpu.zeros_like(dv)
    assert L.spl_vector_permute_dev(n, words, perm.data_ptr(), 0, dv.data_ptr(), fwd.data_ptr(), stream) == 0
    inv = gpu.zeros_like(dv)
    assert L.spl_vector_permute_dev(n, words, perm.data_ptr(), 1, dv.data_ptr(), inv.data_ptr(), stream) == 0
    back = gpu.zeros_like(dv)
    assert L.spl_vector_permute_dev(n, words, perm.data_ptr(), 1, fwd.data_ptr(), back.data_ptr(), stream) == 0
    gpu.cuda.synchronize()
    as_bits = lambda a: np.ascontiguousarray(a).view(np.uint64)  # noqa: E731
    want_inv = np.empty_like(v)
    want_inv[ref.perm] = v
    assert np.array_equal(as_bits(fwd.cpu().numpy()), as_bits(v[ref.perm]))
    assert np.array_equal(as_bits(inv.cpu().numpy()), as_bits(want_inv))
    assert np.array_equal(as_bits(back.cpu().numpy()), as_bits(v))  # inverse after forward: the identity
    if n == 0:  # nothing is touched, pointers or not
        assert L.spl_vector_permute_dev(0, words, None, 0, None, None, None) == 0


# ---- 5. the solve ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.PRECONDITIONERS, ids=lambda k: str(k))
@pytest.mark.parametrize("method,name", CC.SOLVES)
def test_solves_in_the_new_numbering_bit_for_bit(gpu, pkg, method, name, kind):
    S, b = K.matrix(name), np.array(K.rhs(name))
    H = handle_of(pkg, S)
    col = H.coloring(0)
    solver = col.krylov(method, kind)
    if kind == "jacobi":  # the layer makes 1 / diag with torch: the yardstick is given what the device was given
        x_want, want = CC.solve_reference(method, name, kind, solver.solver.parts[1].cpu().numpy())
    else:
        x_want, want = CC.cached_solve_reference(method, name, kind)
    x, res = solver.solve(b, maxiter=2000)
    assert isinstance(x, np.ndarray) and res["converged"], res
    assert (res["iterations"], res["reason"]) == (want.iterations, want.reason), (res["iterations"], want.iterations)
    assert K.bits_equal(res["history"], want.history), int(np.argmax(res["history"] != want.history))
    assert K.bits_equal(x, x_want), float(np.max(np.abs(x - x_want)))
    true = K.true_relative_residual(S, x, b)  # against the ORIGINAL matrix and right-hand side
    print("%s %s %s: %d iterations in the multicolour numbering (%d in the natural one), true relative residual %.2e"
          % (method, name, kind, res["iterations"], K.reference(method, name, kind).iterations, true))
    assert true <= 10 * K.RTOL, true
    # device tensors in, a device tensor out, the same bits; a start vector goes through the permutation too
    tx, tres = solver.solve(dev(gpu, b), maxiter=2000, check_every=5)
    assert tx.is_cuda and K.bits_equal(tx.cpu().numpy(), x_want) and tres["iterations"] == want.iterations
    sx, sres = solver.solve(b, x0=x_want.copy(), maxiter=2000)
    assert sres["converged"] and sres["iterations"] < want.iterations  # from the solution: less work than from zero
    assert K.true_relative_residual(S, sx, b) <= 10 * K.RTOL
    if kind == "ilu0":
        assert solver.ilu.info()["levels"] <= col.ncolors
        if name == "poisson":
            none = CC.cached_solve_reference(method, name, None)[1]
            assert want.iterations < none.iterations, (want.iterations, none.iterations)
    solver.free()
    H.free()


# ---- 6. the Python layer and the threads -------------------------------------------------------------------------------
def test_python_layer(gpu, pkg):
    name = "unsym"
    ref = CC.reference(name, 7)
    S = CC.pattern(name)
    H = handle_of(pkg, S)
    col = H.coloring(seed=7)
    assert col.colors.is_cuda and col.colors.dtype == gpu.int32 and col.perm.is_cuda and col.perm.dtype == gpu.int32
    assert np.array_equal(col.colors.cpu().numpy(), ref.colors) and np.array_equal(col.perm.cpu().numpy(), ref.perm)
    assert isinstance(col.offsets, np.ndarray) and np.array_equal(col.offsets, ref.offsets)
    inf = col.info()
    assert tuple(inf) == pkg.Coloring.INFO_KEYS and col.ncolors == ref.ncolors == inf["colors"]
    assert (inf["n"], inf["rounds"], inf["max_degree"], inf["reserved"]) == (ref.n, ref.rounds, ref.max_degree, 0)
    v = np.array(K.rhs(name))
    moved = col.to_permuted(v)
    assert isinstance(moved, np.ndarray) and K.bits_equal(moved, v[ref.perm])
    assert K.bits_equal(col.from_permuted(moved), v)
    z = dev(gpu, v + 1j * v[::-1])
    tz = col.to_permuted(z)
    assert tz.is_cuda and tz.dtype == gpu.complex128 and np.array_equal(tz.cpu().numpy(), z.cpu().numpy()[ref.perm])
    assert np.array_equal(col.from_permuted(tz).cpu().numpy(), z.cpu().numpy())
    with pytest.raises(pkg.SparseError):
        col.to_permuted(v[:-1])
    with pytest.raises(ValueError):
        col.krylov("gmres")
    # a host Matrix
    C2 = sp.csc_matrix(S)
    C2.sort_indices()
    host = pkg.multicolor(pkg.Matrix(S.shape[1], S.shape[0], C2.indptr, C2.indices, C2.data), seed=7)
    assert np.array_equal(host.colors.cpu().numpy(), ref.colors)
    # not square: refused by the call
    with pytest.raises(pkg.SparseLinearError):
        handle_of(pkg, sp.csr_matrix(np.ones((3, 2)))).coloring()
    H.free()


def test_two_threads_colour_two_handles_at_once(gpu, pkg):
    jobs = [("poisson", 0), ("unsym", 7)]
    handles = [handle_of(pkg, CC.pattern(name)) for name, _ in jobs]
    results, errors = {}, []
    start = threading.Barrier(len(jobs))

    def work(slot):
        try:
            gpu.cuda.set_device(0)
            name, seed = jobs[slot]
            n = CC.reference(name, seed).n
            start.wait()
            results[slot] = [raw_color(pkg, gpu, handles[slot], n, seed) for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for slot, (name, seed) in enumerate(jobs):
        for got in results[slot]:
            assert_is_the_reference(got, CC.reference(name, seed), (name, "thread"))
