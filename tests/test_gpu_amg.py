"""Aggregation AMG on device handles (csrc/amg.hip): spl_matrix_aggregate, spl_amg_*, spl_krylov_set_preconditioner_amg and
the Python layer on them.  The yardstick is the restatement of tests/amg_cases.py (checked on its own in
tests/test_amg_cpu.py): the device's aggregates, roots and round count must equal it EXACTLY, whatever the grid and the
host's check interval are; every level must be the composition of the public handle operations bit for bit; the cycle
and the solves with it must equal the restated cycle on the exported levels bit for bit, with and without the tail
kernel."""
import ctypes as C
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as AK
import coloring_cases as CC
import krylov_cases as K

pytestmark = pytest.mark.gpu

KNOBS = ("SPL_AMG_CHECK_EVERY", "SPL_AMG_GRID", "SPL_AMG_TAIL_ROWS", "SPL_KRYLOV_GRID")
CASES = [(name, seed) for name in CC.NAMES for seed in AK.SEEDS]


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


def scipy_of(H):
    inf = H.info()
    rp, ci, v = H.export_csr()
    return sp.csr_matrix((v, ci, rp), shape=(inf["nrows_global"], inf["ncols"]))


def same_matrix(H, G):
    a, b = H.export_csr(), G.export_csr()
    return H.info()["ncols"] == G.info()["ncols"] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and \
        K.bits_equal(a[2], b[2])


def nan_or_bits_equal(a, b):
    a = np.ascontiguousarray(a).view(np.float64)
    b = np.ascontiguousarray(b).view(np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---- 1. the aggregation ------------------------------------------------------------------------------------------------
def raw_aggregate(pkg, torch, H, n, seed, with_roots=True):
    """spl_matrix_aggregate through ctypes: (agg, roots or None, info)"""
    agg = torch.full((max(n, 1),), -5, dtype=torch.int32, device="cuda")
    roots = torch.full((max(n, 1),), -5, dtype=torch.int32, device="cuda")
    info = (C.c_int64 * 8)(*([-7] * 8))
    torch.cuda.synchronize()
    st = pkg._ffi.lib().spl_matrix_aggregate(H.handle, seed, agg.data_ptr(), roots.data_ptr() if with_roots else None, info)
    assert st == 0, st
    return agg.cpu().numpy()[:n], roots.cpu().numpy() if with_roots else None, list(info)


def assert_is_the_reference(got, ref, what=""):
    agg, roots, info = got
    assert info[:6] + [info[7]] == ref.info(), (what, info, ref.info())
    assert agg.dtype == np.int32 and np.array_equal(agg, ref.agg), (what, "agg", int(np.argmax(agg != ref.agg)) if ref.n else None)
    if roots is not None:
        assert np.array_equal(roots[:ref.count], ref.roots), (what, "roots")
        assert np.all(roots[ref.count:] == -5), (what, "written behind the roots")
    assert (info[6] > 4 * ref.rounds) if ref.n else info[6] == 0, (what, info)


@pytest.mark.parametrize("name,seed", CASES)
def test_aggregates_roots_and_rounds_are_the_restatement(gpu, pkg, name, seed):
    ref = AK.reference(name, seed)
    H = handle_of(pkg, CC.pattern(name))
    assert H.is_complex == (name == "hermitian")
    assert_is_the_reference(raw_aggregate(pkg, gpu, H, ref.n, seed), ref, (name, seed))
    assert_is_the_reference(raw_aggregate(pkg, gpu, H, ref.n, seed, with_roots=False), ref, "bare")  # d_roots is optional
    H.free()


@pytest.mark.parametrize("name", ["poisson", "dense_chain", "chain", "unsym"])
def test_check_interval_and_grid_do_not_show(gpu, pkg, monkeypatch, name):
    seed = 7
    ref = AK.reference(name, seed)
    H = handle_of(pkg, CC.pattern(name))
    launches = {}
    for every in ("1", "4096"):
        for grid in ("1", "3"):
            monkeypatch.setenv("SPL_AMG_CHECK_EVERY", every)
            monkeypatch.setenv("SPL_AMG_GRID", grid)
            got = raw_aggregate(pkg, gpu, H, ref.n, seed)
            assert_is_the_reference(got, ref, (name, every, grid))
            launches[(every, grid)] = got[2][6]
    # the knob was read: rounds are issued in batches, the last ones on a graph without undecided vertices
    assert launches[("1", "1")] == launches[("1", "3")] == 5 + 4 * ref.rounds
    assert launches[("4096", "1")] == 5 + 4 * 4096
    H.free()


# ---- 2. the hierarchy --------------------------------------------------------------------------------------------------
def composed_level(pkg, torch, A, seed, plain):
    """(w, P, R, next A) of the header's recurrence by public DeviceMatrix calls, from the device's own aggregates"""
    cplx = A.is_complex
    n = A.info()["nrows_global"]
    dinv = AK.reciprocal(A.take_diag())
    scaled = A.scale_rows_cols(r=dev(torch, dinv))
    w = AK.weights(AK.omega_of(scaled.norm("inf")), dinv)
    scaled.free()
    g = A.aggregate(seed)
    count = g["info"]["aggregates"]
    ptr = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    ones = torch.ones(n, dtype=torch.complex128 if cplx else torch.float64, device="cuda")
    torch.cuda.synchronize()
    T = pkg.DeviceMatrix.from_csr_dev(n, count, ptr.data_ptr(), g["agg"].data_ptr(), ones.data_ptr(), complex=cplx)
    if plain:
        P = T
    else:
        WA = A.scale_rows_cols(r=dev(torch, w))
        WAT, _ = WA.spgemm(T)
        P = T.lin(1.0, WAT, -1.0)
        for part in (WA, WAT, T):
            part.free()
    R = P.ctrans() if cplx else P.transpose()
    AP, _ = A.spgemm(P)
    RAP, _ = R.spgemm(AP)
    AP.free()
    return w, P, R, RAP


def common_entries(D, S):
    """the values of two CSR matrices of one shape on their common pattern"""
    D, S = sp.csr_matrix(D), sp.csr_matrix(S)
    D.sort_indices()
    S.sort_indices()
    key = lambda M: np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * M.shape[1] + M.indices  # noqa: E731
    _, i, j = np.intersect1d(key(D), key(S), assume_unique=True, return_indices=True)
    return D.data[i], S.data[j]


@pytest.mark.parametrize("plain", [False, True], ids=["smoothed", "plain"])
@pytest.mark.parametrize("coarse", [256, 16])
@pytest.mark.parametrize("name", ["poisson", "hermitian", "unsym", "unsymz"])
def test_every_level_is_the_composition_of_public_calls(gpu, pkg, name, coarse, plain):
    S = K.matrix(name)
    H = handle_of(pkg, S)
    M = H.amg(coarse_size=coarse, plain=plain)
    want = AK.scipy_hierarchy(S, 0, coarse, 16, plain)
    inf = M.info()
    assert M.levels == len(want) == inf["levels"] and inf["n"] == S.shape[0] and inf["coarsest_n"] == want[-1].n
    assert inf["complex"] == np.iscomplexobj(S.data) and not inf["zero_diagonal"] and inf["nnz_fine"] == S.nnz
    A, owned, total = H, [], 0
    for l in range(M.levels):
        got = M.level(l)
        last = l == M.levels - 1
        assert got["dims"] == (want[l].n, 0 if last else want[l + 1].n), (l, got["dims"])
        assert same_matrix(got["A"], A), (l, "A")
        total += got["A"].info()["nnz"]
        if last:
            assert got["P"] is None and got["R"] is None
            dinv = AK.reciprocal(A.take_diag())
            scaled = A.scale_rows_cols(r=dev(gpu, dinv))
            w = AK.weights(AK.omega_of(scaled.norm("inf")), dinv)
            scaled.free()
            assert K.bits_equal(got["w"].cpu().numpy(), w), (l, "w")
            break
        w, P, R, nxt = composed_level(pkg, gpu, A, 0, plain)
        owned += [P, R, nxt]
        assert K.bits_equal(got["w"].cpu().numpy(), w), (l, "w")
        assert same_matrix(got["P"], P) and same_matrix(got["R"], R), (l, "P, R")
        A = nxt
    assert inf["nnz_total"] == total and inf["device_bytes"] > 0
    M.free()
    for part in owned:
        part.free()
    H.free()


@pytest.mark.parametrize("plain", [False, True], ids=["smoothed", "plain"])
@pytest.mark.parametrize("coarse", [256, 16])
@pytest.mark.parametrize("name", ["poisson", "hermitian", "unsym", "unsymz"])
def test_level_values_agree_with_the_scipy_builder(gpu, pkg, name, coarse, plain):
    """every entry of every level's A, P and R on the pattern it shares with the scipy builder's, within 1e-10 relative
    per entry; the level sizes are the restatement's.

    The builder adds the terms of every entry over ascending k, as the header has it (amg_cases._product keeps the rows
    of scipy's products sorted): a level of the 91 x 91 Laplacian has entries whose exact value is zero, and on such an
    entry two evaluations agree relatively only if they add in the same order.  The builder drops an entry that comes
    out as an exact zero where the device stores it, so its pattern lies inside the device's."""
    S = K.matrix(name)
    H = handle_of(pkg, S)
    M = H.amg(coarse_size=coarse, plain=plain)
    want = AK.scipy_hierarchy(S, 0, coarse, 16, plain)
    assert [M.level(l)["dims"][0] for l in range(M.levels)] == [L.n for L in want]
    worst = []
    for l in range(M.levels):
        got = M.level(l)
        for part in ("A", "P", "R"):
            if got[part] is None:
                assert getattr(want[l], part) is None
                continue
            ref = getattr(want[l], part)
            d, s = common_entries(scipy_of(got[part]), ref)
            miss = np.abs(d - s) > 1e-10 * np.abs(s)
            scale = float(np.abs(ref.data).max())
            print("%s level %d %s: %d entries in common of %d / %d, %d beyond 1e-10 relative (largest |reference| among "
                  "them %.3e, largest difference %.3e; largest entry %.3e)"
                  % (name, l, part, len(s), got[part].info()["nnz"], ref.nnz, int(miss.sum()),
                     float(np.abs(s[miss]).max()) if miss.any() else 0.0, float(np.abs(d - s).max()) if len(s) else 0.0, scale))
            worst.append((l, part, int(miss.sum()), len(s), ref.nnz))
    M.free()
    H.free()
    for l, part, missed, common, nnz in worst:
        assert common == nnz, (l, part, common, nnz)  # the builder's pattern is inside the device's
        assert missed == 0, (l, part, missed)


def test_the_pinned_poisson3d(gpu, pkg):
    """poisson3d(16) gives levels 4096 / 404 / 10 with seed 0 and coarse_size 256; operator complexity below 1.5"""
    H = handle_of(pkg, AK.poisson3d(16))
    M = H.amg()
    assert [M.level(l)["dims"][0] for l in range(M.levels)] == [4096, 404, 10]
    assert M.info()["tail_first"] == 1 and 1.0 < M.info()["operator_complexity"] < 1.5
    M.free()
    H.free()


# ---- 3. the cycle ------------------------------------------------------------------------------------------------------
_exported = {}


def exported_levels(pkg, name, coarse):
    """the levels of the default hierarchy as the device built them, exported once: amg_cases.Level objects"""
    if (name, coarse) not in _exported:
        H = handle_of(pkg, K.matrix(name))
        M = H.amg(coarse_size=coarse)
        levels = []
        for l in range(M.levels):
            got = M.level(l)
            levels.append(AK.Level(scipy_of(got["A"]), got["w"].cpu().numpy(), None if got["P"] is None else scipy_of(got["P"]),
                                   None if got["R"] is None else scipy_of(got["R"])))
        M.free()
        H.free()
        _exported[(name, coarse)] = levels
    return _exported[(name, coarse)]


def cycle_inputs(n, cplx):
    """a random vector; finite values whose bits matter (-0.0, subnormals, huge and tiny ones) among ordinary numbers;
    the same with an infinity and a NaN"""
    rng = np.random.default_rng(31 + n + cplx)
    def one():
        v = rng.uniform(-1.0, 1.0, n)
        return v + 1j * rng.uniform(-1.0, 1.0, n) if cplx else v
    plain = one()
    odd = one()
    odd[:6] = [-0.0, 5e-324, 1e300, -1e-300, 0.0, -2.2250738585072014e-308]
    odd[n // 2] = 1e-200
    bad = odd.copy()
    bad[7], bad[n - 1] = np.inf, np.nan
    return plain, odd, bad


@pytest.mark.parametrize("nu,coarse_sweeps", [(1, 4), (2, 1), (1, 1), (2, 4)])
@pytest.mark.parametrize("coarse", [256, 16])
@pytest.mark.parametrize("name", ["poisson", "hermitian"])
def test_cycle_is_the_restatement_with_and_without_the_tail(gpu, pkg, monkeypatch, name, coarse, nu, coarse_sweeps):
    levels = exported_levels(pkg, name, coarse)
    cplx = name == "hermitian"
    ref = AK.Cycle(levels, nu, coarse_sweeps)
    inputs = cycle_inputs(levels[0].n, cplx)
    wants = [ref(b) for b in inputs]
    assert np.all(np.isfinite(wants[0])) and np.all(np.isfinite(wants[1])) and not np.all(np.isfinite(wants[2]))
    H = handle_of(pkg, K.matrix(name))
    count = len(levels)
    sizes = [L.n for L in levels]
    tails = {}
    for rows in ("0", "64", None):
        if rows is not None:
            monkeypatch.setenv("SPL_AMG_TAIL_ROWS", rows)
        else:
            monkeypatch.delenv("SPL_AMG_TAIL_ROWS", raising=False)
        M = H.amg(coarse_size=coarse, sweeps=nu, coarse_sweeps=coarse_sweeps)
        tails[rows] = M.info()["tail_first"]
        for b, want in zip(inputs, wants):
            db = dev(gpu, b)
            dx = gpu.zeros_like(db)
            M.apply_dev(db.data_ptr(), dx.data_ptr(), gpu.cuda.current_stream().cuda_stream)
            gpu.cuda.synchronize()
            got = dx.cpu().numpy()
            assert nan_or_bits_equal(got, want), (rows, float(np.nanmax(np.abs(got - want))))
            assert K.bits_equal(M.apply(dev(gpu, b)).cpu().numpy(), got)  # from call to call, through the layer
        assert K.bits_equal(M.apply(inputs[0]), wants[0])  # host vectors
        M.free()
    small = [l for l in range(count) if all(s <= 64 for s in sizes[l:])]
    assert tails["0"] == -1 and tails["64"] == (small[0] if small else -1)
    assert tails[None] == [l for l in range(count) if all(s <= 1024 for s in sizes[l:])][0]
    if coarse == 16:
        assert sizes == [8281, 1177, 75, 6] and tails["64"] == 3 and tails[None] == 2  # two tail levels, and one
    H.free()


def test_a_hierarchy_that_is_all_tail(gpu, pkg):
    """unsym and unsymz have 300 rows: the whole cycle is the one-workgroup kernel, level 0 included"""
    for name in ("unsym", "unsymz"):
        S = K.matrix(name)
        H = handle_of(pkg, S)
        M = H.amg()
        assert M.info()["tail_first"] == 0 and M.levels == 2
        levels = [AK.Level(scipy_of(g["A"]), g["w"].cpu().numpy(), None if g["P"] is None else scipy_of(g["P"]),
                           None if g["R"] is None else scipy_of(g["R"])) for g in (M.level(l) for l in range(M.levels))]
        b = np.array(K.rhs(name))
        assert K.bits_equal(M.apply(b), AK.Cycle(levels, 1, 4)(b))
        M.free()
        H.free()


def test_two_threads_apply_two_objects_at_once(gpu, pkg):
    names = ["poisson", "hermitian"]
    handles = [handle_of(pkg, K.matrix(name)) for name in names]
    objects = [H.amg(coarse_size=16) for H in handles]
    wants = [AK.Cycle(exported_levels(pkg, name, 16), 1, 4)(np.array(K.rhs(name))) for name in names]
    results, errors = {}, []
    start = threading.Barrier(len(names))

    def work(slot):
        try:
            gpu.cuda.set_device(0)
            b = dev(gpu, K.rhs(names[slot]))
            gpu.cuda.synchronize()
            start.wait()
            with gpu.cuda.stream(gpu.cuda.Stream()):
                results[slot] = [objects[slot].apply(b).cpu().numpy() for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(names))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for slot in range(len(names)):
        for got in results[slot]:
            assert K.bits_equal(got, wants[slot]), names[slot]
    for part in objects + handles:
        part.free()


# ---- 4. Krylov ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,name", K.CASES)
def test_solves_with_the_cycle_bit_for_bit(gpu, pkg, method, name):
    S, b = K.matrix(name), np.array(K.rhs(name))
    H = handle_of(pkg, S)
    M = H.amg()
    levels = [AK.Level(scipy_of(g["A"]), g["w"].cpu().numpy(), None if g["P"] is None else scipy_of(g["P"]),
                       None if g["R"] is None else scipy_of(g["R"])) for g in (M.level(l) for l in range(M.levels))]
    want = K.DRIVERS[method](K._operator(name), b, AK.Cycle(levels, 1, 4), None, K.RTOL, 0.0, 2000)
    solver = H.krylov(method, M)
    assert solver.info()["flags"] & 16 and solver.info()["amg"] and solver.amg is M
    x, res = solver.solve(b, maxiter=2000)
    none = K.reference(method, name, None)
    true = K.true_relative_residual(S, x, b)
    print("%s %s: %d iterations with the cycle (%d without), %d launches an iteration, true relative residual %.2e"
          % (method, name, res["iterations"], none.iterations, solver.info()["launches_per_iteration"], true))
    assert res["converged"] and (res["iterations"], res["reason"]) == (want.iterations, want.reason), (res, want.iterations)
    assert K.bits_equal(res["history"], want.history), int(np.argmax(res["history"] != want.history))
    assert K.bits_equal(x, want.x), float(np.max(np.abs(x - want.x)))
    assert 2 * res["iterations"] <= none.iterations and true <= 1e-7
    assert res["preconditioner_applications"] >= res["iterations"]
    # the look at the status block does not show, device tensors in and out
    tx, tres = solver.solve(dev(gpu, b), maxiter=2000, check_every=3)
    assert tx.is_cuda and K.bits_equal(tx.cpu().numpy(), want.x) and tres["iterations"] == want.iterations
    # each of the two calls clears what the other set
    solver.set_preconditioner("jacobi")
    inf = solver.info()
    assert not inf["amg"] and inf["mid"] and solver.amg is None
    jx, jres = solver.solve(b, maxiter=2000)
    assert jres["converged"] and jres["preconditioner_applications"] > 0
    solver.set_preconditioner(M)
    inf = solver.info()
    assert inf["amg"] and not (inf["T1"] or inf["mid"] or inf["T2"])
    assert K.bits_equal(solver.solve(b, maxiter=2000)[0], want.x)
    assert pkg._ffi.lib().spl_krylov_set_preconditioner_amg(solver.handle, None) == 0 and not solver.info()["flags"] & 30
    solver.free()
    M.free()
    H.free()


def test_a_zero_diagonal_is_a_warning_and_a_non_finite_outcome(gpu, pkg):
    S = sp.lil_matrix(AK.poisson3d(7))  # 343 rows: two levels
    S[100, 100] = 0.0
    Z = sp.csr_matrix(S)
    H = handle_of(pkg, Z)
    M = H.amg()  # SPL_OK: never a refusal
    assert M.info()["zero_diagonal"] and M.levels >= 2
    assert not np.all(np.isfinite(M.level(0)["w"].cpu().numpy()))
    b = np.ones(Z.shape[0])
    for method in ("cg", "bicgstab"):
        solver = H.krylov(method, M)
        x, res = solver.solve(b, maxiter=50)
        assert res["reason"] in (2, 3) and not res["converged"], res
        solver.free()
    M.free()
    H.free()


def test_a_mismatched_cycle_is_refused(gpu, pkg):
    H, G, Z = handle_of(pkg, K.matrix("unsym")), handle_of(pkg, CC.pattern("zeros")), handle_of(pkg, K.matrix("unsymz"))
    M = H.amg()
    for other in (G, Z):  # another size, another value kind
        with pytest.raises(pkg.SparseLinearError) as e:
            other.krylov("bicgstab", M)
        assert e.value.status == pkg._ffi.SPL_ERROR_dimension_mismatch
    with pytest.raises(pkg.SparseLinearError):
        handle_of(pkg, sp.csr_matrix(np.ones((3, 2)))).amg()
    M.free()


# ---- 5. the Python layer -----------------------------------------------------------------------------------------------
def test_python_layer_and_lifetimes(gpu, pkg):
    name = "poisson"
    S, b = K.matrix(name), np.array(K.rhs(name))
    want = K.DRIVERS["cg"](K._operator(name), b, AK.Cycle(exported_levels(pkg, name, 256), 1, 4), None, K.RTOL, 0.0, 2000)
    C2 = sp.csc_matrix(S)
    C2.sort_indices()
    host = pkg.Matrix(S.shape[1], S.shape[0], C2.indptr, C2.indices, C2.data)
    x, res = pkg.cg(host, b, M="amg", maxiter=2000)
    assert res["converged"] and res["iterations"] == want.iterations and K.bits_equal(x, want.x)
    xb, resb = pkg.bicgstab(host, b, M="amg", maxiter=2000)
    assert resb["converged"] and K.true_relative_residual(S, xb, b) <= 1e-7
    M = pkg.amg(host, coarse_size=16)
    assert isinstance(M, pkg.AMG) and M.levels == 4 and tuple(M.info())[:8] == pkg.AMG.INFO_KEYS
    lvl = M.level(1)
    assert lvl["dims"] == (1177, 75) and lvl["w"].is_cuda and lvl["w"].dtype == gpu.float64 and lvl["w"].shape == (1177,)
    assert lvl["A"].info()["nrows_global"] == 1177 and lvl["P"].info()["ncols"] == 75 and lvl["R"].info()["nrows_global"] == 75
    lvl["A"].free()  # a view: the level stays
    assert M.level(1)["A"].info()["nnz"] == lvl["A"].info()["nnz"]
    with pytest.raises(pkg.SparseLinearError):
        M.level(4)
    with pytest.raises(pkg.SparseError):
        M.apply(b[:-1])
    g = M.A.aggregate(seed=7)
    ref = AK.reference(name, 7)
    assert g["agg"].dtype == gpu.int32 and g["agg"].is_cuda and np.array_equal(g["agg"].cpu().numpy(), ref.agg)
    assert np.array_equal(g["roots"].cpu().numpy(), ref.roots) and g["info"]["aggregates"] == ref.count
    assert tuple(g["info"]) == pkg.AMG.AGGREGATE_KEYS
    # an AMG kept alive by its solver, and one AMG for two solvers
    def make():
        A = host.device_handle()
        return A.krylov("cg", A.amg()), A.krylov("bicgstab", "amg")
    first, second = make()
    import gc
    gc.collect()
    assert K.bits_equal(first.solve(b, maxiter=2000)[0], want.x)
    shared = first.amg
    other = first.A.krylov("bicgstab", shared)
    assert other.solve(b, maxiter=2000)[1]["converged"] and second.solve(b, maxiter=2000)[1]["converged"]
    owned = second.amg
    second.free()  # the one "amg" built goes with its solver
    with pytest.raises(pkg.SparseLinearError):
        owned.info()
    assert shared.info()["levels"] == 3  # a borrowed one stays
    for part in (first, other, shared, M):
        part.free()
    with pytest.raises(ValueError):
        host.device_handle().krylov("cg", "multigrid")
