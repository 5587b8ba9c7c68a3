"""The order in which the spl_lobpcg_* entry points refuse their arguments (csrc/abi.hip), called raw through ctypes on
an 8 x 8 Hermitian positive definite tridiagonal handle, real and complex, in the manner of
tests/test_gpu_solver_refusals.py: every refused call breaks TWO rules, the one whose status is expected and one further
down the ladder of include/sparse_linear_hip.h, so the tables pin the order and not only the set."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_solver_refusals import ARG, DIM, HANDLE, N, NAN, NEG, OK, OVERFLOW, TWO31, handle_of, p, tridiagonal, vp

pytestmark = pytest.mark.gpu

MATRIX = -8  # SPL_ERROR_invalid_matrix
BLOCK = 2


class World:
    def __init__(self, pkg, torch, cplx):
        self.L = L = pkg._ffi.lib()
        self.cplx = cplx
        self.A = handle_of(pkg, tridiagonal(N, cplx))
        self.A7 = handle_of(pkg, tridiagonal(N - 1, cplx))
        self.owned = []
        self.solver = self.make(L.spl_lobpcg_create, L.spl_lobpcg_free, self.A.handle, BLOCK)
        self.tri = self.make(L.spl_trisolve_analyze, L.spl_trisolve_free, self.A.handle, 0, 0)
        self.tri7 = self.make(L.spl_trisolve_analyze, L.spl_trisolve_free, self.A7.handle, 0, 0)
        self.amg = self.make(L.spl_amg_create, L.spl_amg_free, self.A.handle, None)
        self.amg7 = self.make(L.spl_amg_create, L.spl_amg_free, self.A7.handle, None)
        dtype = torch.complex128 if cplx else torch.float64
        rng = np.random.default_rng(3)
        start = rng.standard_normal(2 * BLOCK * N)
        self.vec = torch.from_numpy(start[:BLOCK * N] + (1j * start[BLOCK * N:] if cplx else 0.0)).to(dtype).cuda()
        self.out = torch.zeros(BLOCK * N, dtype=dtype, device="cuda")
        self.entry = 16 if cplx else 8
        self.host = np.ascontiguousarray(self.vec.cpu().numpy())

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


def solve(W, dev, handle="self", nev=1, which=1, tol=1e-8, atol=0.0, max_iter=5, x0="x0", ldx0=N, values=True, vectors="out",
          ldx=N, residuals=True, result=True, history=False):
    h = {"self": W.solver, "matrix": W.A.handle, "null": None}[handle]
    vals, res = np.full(BLOCK, -7.0), np.full(BLOCK, -7.0)
    out = (C.c_int64 * 8)(*([-7] * 8))
    hist = np.full(8, -7.0)
    hv = np.zeros(2 * BLOCK * N)
    if dev:
        ptr = {"x0": W.vec.data_ptr(), "out": W.out.data_ptr(), "null": None, "off": W.vec.data_ptr() + W.entry // 2}
    else:
        ptr = {"x0": p(W.host.view(np.float64)), "out": p(hv), "null": None, "off": p(W.host.view(np.float64))}
    args = (h, nev, which, tol, atol, max_iter, ptr[x0], ldx0, p(vals) if values else None, ptr[vectors], ldx,
            p(res) if residuals else None, out if result else None, p(hist) if history else None)
    st = W.L.spl_lobpcg_solve_dev(*args, None) if dev else W.L.spl_lobpcg_solve(*args)
    return st, list(out), vals, hist


@pytest.mark.parametrize("dev", [True, False], ids=["dev", "host"])
def test_solve_refuses_in_the_header_s_order(W, dev):
    ladder = [
        (dict(handle="matrix", values=False), HANDLE),            # the handle before the outputs
        (dict(handle="null", max_iter=-1), HANDLE),
        (dict(values=False, max_iter=-1), ARG),                    # the outputs before max_iter
        (dict(residuals=False, max_iter=-1), ARG),
        (dict(result=False, max_iter=-1), ARG),
        (dict(max_iter=-1, nev=0), NEG),                           # max_iter before the scalars
        (dict(nev=0, max_iter=TWO31, history=True), ARG),          # the scalars before the history's length
        (dict(nev=BLOCK + 1, max_iter=TWO31, history=True), ARG),
        (dict(which=2, max_iter=TWO31, history=True), ARG),        # largest magnitude is refused
        (dict(which=-1, max_iter=TWO31, history=True), ARG),
        (dict(tol=-1.0, max_iter=TWO31, history=True), ARG),
        (dict(tol=NAN, max_iter=TWO31, history=True), ARG),
        (dict(atol=-1.0, max_iter=TWO31, history=True), ARG),
        (dict(atol=NAN, max_iter=TWO31, history=True), ARG),
        (dict(max_iter=TWO31, history=True, x0="null"), OVERFLOW),  # the history's length before the vectors
        (dict(max_iter=TWO31, history=True, ldx=N - 1), OVERFLOW),
        (dict(x0="null"), ARG),
        (dict(vectors="null"), ARG),
        (dict(ldx0=N - 1), ARG),
        (dict(ldx=N - 1), ARG),
    ]
    if dev:
        ladder += [(dict(x0="off"), ARG), (dict(vectors="off"), ARG)]
    for bad, status in ladder:
        st, out, vals, hist = solve(W, dev, **bad)
        assert st == status, (bad, st, status)
        assert out == [-7] * 8 and (vals == -7.0).all() and (hist == -7.0).all(), bad  # nothing was written
    st, out, vals, hist = solve(W, dev, nev=BLOCK, history=True)
    assert st == OK and out[0] in (0, 1) and out[3] == BLOCK and (vals != -7.0).all()
    st, out, _, _ = solve(W, dev, max_iter=0)  # allowed: the check of iteration 0 ends the solve
    assert st == OK and out[:2] == [1, 0]


def test_a_block_wider_than_the_matrix_is_refused_by_the_solve(W, pkg):
    h = vp()
    tiny = handle_of(pkg, tridiagonal(2, W.cplx))
    assert W.L.spl_lobpcg_create(tiny.handle, 3, C.byref(h)) == OK  # create does not compare the block with n
    vals = np.zeros(4)
    out = (C.c_int64 * 8)()
    assert W.L.spl_lobpcg_solve_dev(h, 1, 1, 1e-8, 0.0, 5, W.vec.data_ptr(), 2, p(vals), W.out.data_ptr(), 2, p(vals), out,
                                    None, None) == ARG
    W.L.spl_lobpcg_free(C.byref(h))
    W.L.spl_lobpcg_free(C.byref(h))  # idempotent
    assert not h.value


def test_create_refuses_in_the_header_s_order(W, pkg):
    L = W.L
    junk = C.create_string_buffer(256)
    h = vp(7)
    assert L.spl_lobpcg_create(junk, 0, None) == HANDLE                     # the handle before L and the block
    assert L.spl_lobpcg_create(W.A.handle, 0, None) == ARG
    wide = sp.csc_matrix(np.ones((2, 3)) + (0j if W.cplx else 0.0))
    Hw = handle_of(pkg, wide)
    for block in (0, 43, -1):
        h = vp(7)
        assert L.spl_lobpcg_create(Hw.handle, block, C.byref(h)) == ARG and not h.value  # the block before the shape
    assert L.spl_lobpcg_create(Hw.handle, 2, C.byref(h)) == DIM and not h.value          # the shape before the values
    skew = sp.csc_matrix(np.array([[2.0, 1.0], [0.5, 2.0]]) + (0j if W.cplx else 0.0))
    assert L.spl_lobpcg_create(handle_of(pkg, skew).handle, 1, C.byref(h)) == MATRIX and not h.value
    assert L.spl_lobpcg_create(W.A.handle, 42, C.byref(h)) == OK and h.value
    info = (C.c_int64 * 8)()
    assert L.spl_lobpcg_info(h, info) == OK and list(info)[:3] == [N, 42, 1 if W.cplx else 0]
    assert L.spl_lobpcg_info(h, None) == ARG and L.spl_lobpcg_info(W.A.handle, None) == HANDLE
    L.spl_lobpcg_free(C.byref(h))
    assert not h.value


def test_the_setters_refuse_in_the_krylov_calls_order(W):
    L = W.L
    off = W.vec.data_ptr() + W.entry // 2
    junk = C.create_string_buffer(256)
    assert L.spl_lobpcg_set_preconditioner(W.A.handle, junk, off, None) == HANDLE   # L before the parts
    assert L.spl_lobpcg_set_preconditioner(W.solver, junk, off, W.tri7) == HANDLE   # a part that is none before the rest
    assert L.spl_lobpcg_set_preconditioner(W.solver, W.tri7, off, None) == ARG      # the alignment before the sizes
    assert L.spl_lobpcg_set_preconditioner(W.solver, W.tri, None, W.tri7) == DIM
    assert L.spl_lobpcg_set_preconditioner(W.solver, W.tri, W.vec.data_ptr(), W.tri) == OK
    info = (C.c_int64 * 8)()
    assert L.spl_lobpcg_info(W.solver, info) == OK and info[2] == (1 if W.cplx else 0) | 2 | 4 | 8
    assert L.spl_lobpcg_set_preconditioner_amg(W.A.handle, junk) == HANDLE
    assert L.spl_lobpcg_set_preconditioner_amg(W.solver, junk) == HANDLE
    assert L.spl_lobpcg_set_preconditioner_amg(W.solver, W.amg7) == DIM
    assert L.spl_lobpcg_set_preconditioner_amg(W.solver, W.amg) == OK                # clears the parts
    assert L.spl_lobpcg_info(W.solver, info) == OK and info[2] == (1 if W.cplx else 0) | 16
    assert L.spl_lobpcg_set_preconditioner_amg(W.solver, None) == OK
    assert L.spl_lobpcg_info(W.solver, info) == OK and info[2] == (1 if W.cplx else 0)
