"""The order in which the iterative objects behind handles refuse their arguments (csrc/abi.hip), called raw through
ctypes: CG, BiCGSTAB, GMRES and Lanczos on an 8 x 8 Hermitian positive definite tridiagonal handle, real and complex.
Every refused call breaks TWO rules, the one whose status is expected and one further down the ladder, so the tables pin
the order and not only the set.  Where two rules share a status the object with n == 0 tells them apart: its early
return lies between the checks of the scalars and the checks of the vectors.  Plus the setters of the
preconditioner, the object with n == 0, and spl_*_free on NULL, on a pointer to NULL and twice on one handle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

OK = 0
HANDLE = -3       # SPL_ERROR_invalid_handle
ARG = -5          # SPL_ERROR_argument_missing
NEG = -6          # SPL_ERROR_n_nonpositive
DIM = -20         # SPL_ERROR_dimension_mismatch
OVERFLOW = -22    # SPL_ERROR_index_overflow

N = 8
NAN = float("nan")
TWO31 = 1 << 31
vp = C.c_void_p
LINEAR = ["cg", "bicgstab", "gmres"]


def tridiagonal(n, cplx):
    off = (-1.0 + 0.5j) if cplx else -1.0
    S = sp.diags([np.full(n - 1, np.conj(off)), np.full(n, 4.0 + 0j if cplx else 4.0), np.full(n - 1, off)], [-1, 0, 1])
    return sp.csc_matrix(S)


def handle_of(pkg, S):
    if S.shape[0] == 0:
        return pkg.DeviceMatrix.ident(0)
    S.sort_indices()
    M = pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)
    return pkg.DeviceMatrix.from_csc_complex(M) if np.iscomplexobj(S.data) else pkg.DeviceMatrix.from_csc(M)


def p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class World:
    """the handles, objects and vectors of one value kind; everything is freed by close()"""

    def __init__(self, pkg, torch, cplx):
        self.L = L = pkg._ffi.lib()
        self.cplx = cplx
        self.A = handle_of(pkg, tridiagonal(N, cplx))
        self.A7 = handle_of(pkg, tridiagonal(N - 1, cplx))
        self.A0 = pkg.DeviceMatrix.ident(0)
        self.owned = []  # (free function, handle)
        self.cg = self.make(L.spl_krylov_create, L.spl_krylov_free, self.A.handle, 0)
        self.bicgstab = self.make(L.spl_krylov_create, L.spl_krylov_free, self.A.handle, 1)
        self.gmres = self.make(L.spl_gmres_create, L.spl_gmres_free, self.A.handle, 5)
        self.eigsh = self.make(L.spl_eigsh_create, L.spl_eigsh_free, self.A.handle, 4)
        self.cg7 = self.make(L.spl_krylov_create, L.spl_krylov_free, self.A7.handle, 0)
        self.cg0 = self.make(L.spl_krylov_create, L.spl_krylov_free, self.A0.handle, 0)
        self.bicgstab0 = self.make(L.spl_krylov_create, L.spl_krylov_free, self.A0.handle, 1)
        self.gmres0 = self.make(L.spl_gmres_create, L.spl_gmres_free, self.A0.handle, 5)
        self.tri = self.make(L.spl_trisolve_analyze, L.spl_trisolve_free, self.A.handle, 0, 0)
        self.tri7 = self.make(L.spl_trisolve_analyze, L.spl_trisolve_free, self.A7.handle, 0, 0)
        self.amg = self.make(L.spl_amg_create, L.spl_amg_free, self.A.handle, None)
        self.amg7 = self.make(L.spl_amg_create, L.spl_amg_free, self.A7.handle, None)
        dtype = torch.complex128 if cplx else torch.float64
        self.vec = torch.ones(4 * N, dtype=dtype, device="cuda")  # b, x and the columns of eigsh
        self.entry = 16 if cplx else 8
        self.b = self.vec.data_ptr()
        self.x = self.b + N * self.entry
        self.off = self.b + self.entry // 2  # not a whole entry from the start

    def make(self, create, free, *args):
        h = vp()
        assert create(*args, C.byref(h)) == OK and h.value
        self.owned.append((free, h))
        return h

    def close(self):
        for free, h in reversed(self.owned):
            free(C.byref(h))
            assert not h.value


@pytest.fixture(scope="module", params=[False, True], ids=["real", "complex"])
def W(request, pkg, gpu):
    w = World(pkg, gpu, request.param)
    yield w
    w.close()


# ---- the solve calls of CG, BiCGSTAB and GMRES ---------------------------------------------------------------------------
def linear_call(W, name, dev, handle="self", b="b", x="x", rtol=1e-8, atol=0.0, max_iter=5, check_every=0, result=True,
                residual=True, history=False, empty=False):
    """one solve call of `name`, through the device entry point or the host one; returns (status, result, residual, hist)"""
    L = W.L
    obj = getattr(W, name + ("0" if empty else ""))
    h = {"self": obj, "matrix": W.A.handle, "null": None}[handle]
    res = (C.c_int64 * 6)(*([-7] * 6))
    rsd = np.full(2, -7.0)
    hist = np.full(8, -7.0)
    hb = np.ones(2 * N)
    hx = np.zeros(2 * N)
    if dev:
        ptr = {"b": W.b, "x": W.x, "null": None, "off": W.off}
        vb, vx = ptr[b], ptr[x]
    else:
        ptr = {"b": p(hb), "x": p(hx), "null": None, "off": p(hb)}
        vb, vx = ptr[b], ptr[x]
    common = (h, vb, vx, 0, rtol, atol, max_iter) + ((check_every,) if dev else ())
    outs = (res if result else None, p(hist) if history else None)
    if name == "gmres":
        fn = L.spl_gmres_solve_dev if dev else L.spl_gmres_solve
        args = common + outs + (p(rsd) if residual else None,) + ((None,) if dev else ())
    else:
        fn = L.spl_krylov_solve_dev if dev else L.spl_krylov_solve
        args = common + outs + ((None,) if dev else ())
    return fn(*args), list(res), rsd.tolist(), hist


# (label, the two rules broken, status).  The ladder: handle, outputs, max_iter, tolerances / check_every, history's
# length, [n == 0 returns], vectors given and apart, vectors aligned
SCALAR_LADDER = [
    ("matrix handle + NULL result", dict(handle="matrix", result=False), HANDLE),
    ("NULL handle + max_iter < 0", dict(handle="null", max_iter=-1), HANDLE),
    ("NULL result + max_iter < 0", dict(result=False, max_iter=-1), ARG),
    ("max_iter < 0 + NaN rtol", dict(max_iter=-1, rtol=NAN), NEG),
    ("max_iter < 0 + long history", dict(max_iter=-1, history=True), NEG),
    ("NaN rtol + long history", dict(rtol=NAN, history=True, max_iter=TWO31), ARG),
    ("negative atol + long history", dict(atol=-1.0, history=True, max_iter=TWO31), ARG),
    ("NaN rtol + aliased vectors", dict(rtol=NAN, x="b"), ARG),
    ("long history + NULL b", dict(history=True, max_iter=TWO31, b="null"), OVERFLOW),
]
DEVICE_ONLY = [
    ("check_every < 0 + long history", dict(check_every=-1, history=True, max_iter=TWO31), ARG),
    ("NULL b + misaligned x", dict(b="null", x="off"), ARG),
    ("aliased vectors", dict(x="b"), ARG),
    ("misaligned b", dict(b="off"), ARG),
    ("misaligned x", dict(x="off"), ARG),
]
HOST_ONLY = [
    ("NULL b", dict(b="null"), ARG),
    ("NULL x", dict(x="null"), ARG),
]
GMRES_ONLY = [
    ("NULL residual + max_iter < 0", dict(residual=False, max_iter=-1), ARG),
    ("matrix handle + NULL residual", dict(handle="matrix", residual=False), HANDLE),
]


def ladder(name, dev):
    return SCALAR_LADDER + (DEVICE_ONLY if dev else HOST_ONLY) + (GMRES_ONLY if name == "gmres" else [])


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "host"])
@pytest.mark.parametrize("name", LINEAR)
def test_linear_solve_ladder(W, name, dev):
    for label, broken, status in ladder(name, dev):
        st, res, rsd, hist = linear_call(W, name, dev, **broken)
        assert st == status, (label, st)
        # refused before anything is written
        if broken.get("result", True):
            assert res == [-7] * 6, label
        assert rsd == [-7.0, -7.0] and hist[0] == -7.0, label


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "host"])
@pytest.mark.parametrize("name", LINEAR)
def test_empty_object_returns_between_scalars_and_vectors(W, name, dev):
    """n == 0: the scalars are still checked (the statuses of the ladder, nothing written), the vectors are not"""
    for label, broken, status in SCALAR_LADDER + (GMRES_ONLY if name == "gmres" else []):
        if broken.get("handle", "self") != "self":
            continue
        st, res, rsd, hist = linear_call(W, name, dev, empty=True, **broken)
        assert st == status, (label, st)
        if broken.get("result", True):
            assert res == [-7] * 6, label
    nres = 6 if name == "gmres" else 4
    for broken in (dict(b="null", x="null"), dict(x="b"), dict(b="off") if dev else dict(b="null")):
        st, res, rsd, hist = linear_call(W, name, dev, empty=True, history=True, **broken)
        assert st == OK, broken
        assert res[:nres] == [0] * nres and hist[0] == 0.0 and hist[1] == -7.0, broken
        assert rsd == ([0.0, 0.0] if name == "gmres" else [-7.0, -7.0]), broken
    st, res, _, _ = linear_call(W, name, dev, empty=True, history=False, b="null", x="null")
    assert st == OK and res[:nres] == [0] * nres


@pytest.mark.parametrize("name", LINEAR)
def test_host_call_takes_aliased_vectors(W, name):
    """the host entry points copy b up before x comes down: b == x is served, as is any alignment"""
    L = W.L
    bx = np.ones(2 * N)
    rhs = bx.view(np.complex128)[:N].copy() if W.cplx else bx[:N].copy()
    res = (C.c_int64 * 6)(*([-7] * 6))
    rsd = np.full(2, -7.0)
    if name == "gmres":
        st = L.spl_gmres_solve(W.gmres, p(bx), p(bx), 0, 1e-10, 0.0, 50, res, None, p(rsd))
    else:
        st = L.spl_krylov_solve(getattr(W, name), p(bx), p(bx), 0, 1e-10, 0.0, 50, res, None)
    assert st == OK and res[1] == 0 and 0 < res[0] <= 50
    x = bx.view(np.complex128)[:N] if W.cplx else bx[:N]
    assert np.allclose(tridiagonal(N, W.cplx) @ x, rhs, rtol=1e-8, atol=0)


# ---- Lanczos ------------------------------------------------------------------------------------------------------------
def eigsh_call(W, dev, handle="self", nev=1, which=0, tol=1e-8, atol=0.0, max_restarts=5, v0="b", vectors="x", ldx=N,
               values=True, residuals=True, result=True, history=False):
    L = W.L
    h = {"self": W.eigsh, "matrix": W.A.handle, "null": None}[handle]
    val, rsd, hist = np.full(4, -7.0), np.full(4, -7.0), np.full(8, -7.0)
    res = (C.c_int64 * 6)(*([-7] * 6))
    hv0, hvec = np.ones(2 * N), np.zeros(4 * N)
    ptr = ({"b": W.b, "x": W.x, "null": None, "off": W.off} if dev else
           {"b": p(hv0), "x": p(hvec), "null": None, "off": p(hv0)})
    fn = L.spl_eigsh_solve_dev if dev else L.spl_eigsh_solve
    st = fn(h, nev, which, tol, atol, max_restarts, ptr[v0], p(val) if values else None, ptr[vectors], ldx,
            p(rsd) if residuals else None, res if result else None, p(hist) if history else None, *((None,) if dev else ()))
    return st, list(res), val, rsd, hist


# the ladder: handle, outputs, max_restarts, nev / which / tolerances, history's length, vectors given and ldx, aligned
EIGSH_LADDER = [
    ("matrix handle + NULL values", dict(handle="matrix", values=False), HANDLE),
    ("NULL handle + max_restarts < 1", dict(handle="null", max_restarts=0), HANDLE),
    ("NULL values + max_restarts < 1", dict(values=False, max_restarts=0), ARG),
    ("NULL residuals + max_restarts < 1", dict(residuals=False, max_restarts=0), ARG),
    ("NULL result + max_restarts < 1", dict(result=False, max_restarts=0), ARG),
    ("max_restarts < 1 + nev < 1", dict(max_restarts=0, nev=0), NEG),
    ("max_restarts < 1 + long history", dict(max_restarts=-3, history=True), NEG),
    ("nev < 1 + long history", dict(nev=0, history=True, max_restarts=TWO31), ARG),
    ("nev >= ncv + long history", dict(nev=4, history=True, max_restarts=TWO31), ARG),
    ("which out of range + long history", dict(which=3, history=True, max_restarts=TWO31), ARG),
    ("NaN tol + long history", dict(tol=NAN, history=True, max_restarts=TWO31), ARG),
    ("negative atol + long history", dict(atol=-1.0, history=True, max_restarts=TWO31), ARG),
    ("long history + NULL v0", dict(history=True, max_restarts=TWO31, v0="null"), OVERFLOW),
    ("long history + short ldx", dict(history=True, max_restarts=TWO31, ldx=N - 1), OVERFLOW),
    ("NULL v0", dict(v0="null"), ARG),
    ("NULL vectors", dict(vectors="null"), ARG),
    ("short ldx", dict(ldx=N - 1), ARG),
]
EIGSH_DEVICE_ONLY = [
    ("NULL v0 + misaligned vectors", dict(v0="null", vectors="off"), ARG),
    ("misaligned v0", dict(v0="off"), ARG),
    ("misaligned vectors", dict(vectors="off"), ARG),
]


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "host"])
def test_eigsh_solve_ladder(W, dev):
    for label, broken, status in EIGSH_LADDER + (EIGSH_DEVICE_ONLY if dev else []):
        st, res, val, rsd, hist = eigsh_call(W, dev, **broken)
        assert st == status, (label, st)
        if broken.get("result", True):
            assert res == [-7] * 6, label
        assert val[0] == -7.0 and rsd[0] == -7.0 and hist[0] == -7.0, label


def test_eigsh_set_inverse_ladder(W):
    L = W.L
    cases = [
        ("matrix handle + matrix as K", (W.A.handle, W.A.handle, 0.0, 1e-8, 0.0, 5), HANDLE),
        ("NULL handle", (None, W.cg, 0.0, 1e-8, 0.0, 5), HANDLE),
        ("matrix as K + max_iter < 0", (W.eigsh, W.A.handle, 0.0, 1e-8, 0.0, -1), HANDLE),
        ("GMRES as K", (W.eigsh, W.gmres, 0.0, 1e-8, 0.0, 5), HANDLE),
        ("K of size 7 + max_iter < 0", (W.eigsh, W.cg7, 0.0, 1e-8, 0.0, -1), DIM),
        ("max_iter < 0 + NaN rtol", (W.eigsh, W.cg, 0.0, NAN, 0.0, -1), NEG),
        ("NaN rtol", (W.eigsh, W.cg, 0.0, NAN, 0.0, 5), ARG),
        ("negative atol", (W.eigsh, W.cg, 0.0, 1e-8, -1.0, 5), ARG),
        ("sigma not finite", (W.eigsh, W.cg, float("inf"), 1e-8, 0.0, 5), ARG),
    ]
    info = (C.c_int64 * 8)()
    for label, args, status in cases:
        assert L.spl_eigsh_set_inverse(*args) == status, label
        assert L.spl_eigsh_info(W.eigsh, info) == OK and info[2] == (1 if W.cplx else 0), label  # nothing was set
    assert L.spl_eigsh_set_inverse(W.eigsh, W.cg, 0.5, 1e-8, 0.0, 5) == OK
    assert L.spl_eigsh_info(W.eigsh, info) == OK and info[2] == (1 if W.cplx else 0) | 2
    # NULL takes the solver away and looks at nothing else
    assert L.spl_eigsh_set_inverse(W.eigsh, None, NAN, NAN, -1.0, -1) == OK
    assert L.spl_eigsh_info(W.eigsh, info) == OK and info[2] == (1 if W.cplx else 0)


# ---- the setters of the preconditioner -----------------------------------------------------------------------------------
def setters(W, name):
    L = W.L
    if name == "gmres":
        return W.gmres, L.spl_gmres_set_preconditioner, L.spl_gmres_set_preconditioner_amg, L.spl_gmres_info
    return getattr(W, name), L.spl_krylov_set_preconditioner, L.spl_krylov_set_preconditioner_amg, L.spl_krylov_info


@pytest.mark.parametrize("name", LINEAR)
def test_set_preconditioner_ladder(W, name):
    """the ladder: solver handle, part handles, d_mid aligned to whole entries, size / kind / device of the parts"""
    S, set_parts, set_amg, info_fn = setters(W, name)
    mid = W.b
    half = W.b + 8  # a double further: no whole entry of the complex object
    width = 1 if W.cplx else 0
    info = (C.c_int64 * 8)()

    def flags():
        assert info_fn(S, info) == OK
        return info[2]

    cases = [
        ("matrix as the solver + matrix as a part", (W.A.handle, W.A.handle, mid, None), HANDLE),
        ("NULL solver + part of size 7", (None, W.tri7, mid, None), HANDLE),
        ("matrix as T1 + part of size 7", (S, W.A.handle, mid, W.tri7), HANDLE),
        ("matrix as T2 + part of size 7", (S, W.tri7, mid, W.A.handle), HANDLE),
        ("a solver as a part", (S, S, mid, None), HANDLE),
        ("part of size 7", (S, W.tri7, mid, None), DIM),
        ("part of size 7 behind a good one", (S, W.tri, mid, W.tri7), DIM),
    ]
    if W.cplx:
        cases += [
            ("matrix as a part + d_mid off by 8", (S, W.A.handle, half, None), HANDLE),
            ("d_mid off by 8 + part of size 7", (S, W.tri7, half, None), ARG),
            ("d_mid off by 8", (S, W.tri, half, W.tri), ARG),
        ]
    else:
        cases += [("d_mid off by 4 + part of size 7", (S, W.tri7, W.b + 4, None), ARG)]
    for label, args, status in cases:
        assert set_parts(*args) == status, label
        assert flags() == width, label  # nothing was set
    assert set_parts(S, W.tri, mid, W.tri) == OK and flags() == width | 2 | 4 | 8
    amg_cases = [
        ("matrix as the solver + matrix as M", (W.A.handle, W.A.handle), HANDLE),
        ("NULL solver + M of size 7", (None, W.amg7), HANDLE),
        ("matrix as M", (S, W.A.handle), HANDLE),
        ("a triangular solver as M", (S, W.tri), HANDLE),
        ("M of size 7", (S, W.amg7), DIM),
    ]
    for label, args, status in amg_cases:
        assert set_amg(*args) == status, label
        assert flags() == width | 2 | 4 | 8, label  # the parts stay
    assert set_amg(S, W.amg) == OK and flags() == width | 16
    assert set_parts(S, None, mid, None) == OK and flags() == width | 4
    assert set_amg(S, None) == OK and flags() == width
    assert set_parts(S, None, None, None) == OK and flags() == width


@pytest.mark.parametrize("name", LINEAR)
def test_setters_refuse_a_freed_solver(W, name):
    L = W.L
    create, free = ((L.spl_gmres_create, L.spl_gmres_free) if name == "gmres" else (L.spl_krylov_create, L.spl_krylov_free))
    h = vp()
    assert create(W.A.handle, 5 if name == "gmres" else LINEAR.index(name), C.byref(h)) == OK
    stale = vp(h.value)
    free(C.byref(h))
    assert not h.value
    _, set_parts, set_amg, info_fn = setters(W, name)
    assert set_parts(stale, W.tri7, W.b, None) == HANDLE  # before the part of size 7 is looked at
    assert set_amg(stale, W.amg7) == HANDLE
    assert info_fn(stale, (C.c_int64 * 8)()) == HANDLE


# ---- spl_*_free ----------------------------------------------------------------------------------------------------------
def test_free_on_null_and_twice(W):
    L = W.L
    A = W.A.handle
    makers = [
        (L.spl_matrix_free, lambda h: L.spl_matrix_transpose(A, C.byref(h))),
        (L.spl_trisolve_free, lambda h: L.spl_trisolve_analyze(A, 0, 0, C.byref(h))),
        (L.spl_ilu0_free, lambda h: L.spl_ilu0_analyze(A, C.byref(h))),
        (L.spl_krylov_free, lambda h: L.spl_krylov_create(A, 0, C.byref(h))),
        (L.spl_amg_free, lambda h: L.spl_amg_create(A, None, C.byref(h))),
        (L.spl_gmres_free, lambda h: L.spl_gmres_create(A, 5, C.byref(h))),
        (L.spl_eigsh_free, lambda h: L.spl_eigsh_create(A, 4, C.byref(h))),
    ]
    for free, make in makers:
        free(None)
        empty = vp()
        free(C.byref(empty))
        assert not empty.value
        h = vp()
        assert make(h) == OK and h.value
        free(C.byref(h))
        assert not h.value
        free(C.byref(h))
        assert not h.value
    # a handle of another kind is not freed, and the caller's pointer is cleared all the same
    other = vp()
    assert L.spl_krylov_create(A, 0, C.byref(other)) == OK
    keep = vp(other.value)
    L.spl_gmres_free(C.byref(other))
    assert not other.value
    info = (C.c_int64 * 8)()
    assert L.spl_krylov_info(keep, info) == OK and info[0] == N
    L.spl_krylov_free(C.byref(keep))
    assert not keep.value
