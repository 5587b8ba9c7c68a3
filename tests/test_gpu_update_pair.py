"""spl_vector_update_pair_dev alone (csrc/basis_pair.hpp): the update of a column and of its image under B by the same
coefficients in one launch, with Re<w, bw> of the results.  w and bw must equal a numpy restatement (one product and one
difference per term, ascending) bit for bit; *d_q must equal the real part of what the EXISTING spl_vector_dot_dev writes
for the results, so the yardstick of the reduction is not the new code.  Padded leading dimensions; rows from n on and
the columns of V and BV are untouched; d_q == NULL and SPL_KRYLOV_GRID leave the bits alone.  Then the refusals."""
import ctypes as C

import numpy as np
import pytest

import globpcg_cases as GK
import krylov_cases as K
from test_gpu_eigsh import dev

pytestmark = pytest.mark.gpu

OK, ARG, NEG = 0, -5, -6
SIZES = (0, 1, 255, 4096, 4097, 8209)  # one entry, a part chunk, a whole chunk, one entry more, three chunks
COLUMNS = (1, 5, 128)
TAIL = 7  # entries behind w and bw that the kernel must leave alone
_cases = {}


@pytest.fixture(autouse=True)
def default_grid(monkeypatch):
    monkeypatch.delenv("SPL_KRYLOV_GRID", raising=False)


def case_of(n, k, cplx):
    """V, BV (k columns, ldv = n + 3 and ldbv = n + 5 entries apart, NaN between them), the coefficients, w, bw, and the
    restated results; computed once"""
    key = (n, k, cplx)
    if key not in _cases:
        rng = np.random.default_rng(7 * n + 131 * k + cplx)
        dtype = np.complex128 if cplx else np.float64

        def draw(count):
            a = rng.standard_normal(count)
            return (a + 1j * rng.standard_normal(count)).astype(dtype) if cplx else a

        ldv, ldbv = n + 3, n + 5
        V, BV = np.full(k * ldv, np.nan, dtype=dtype), np.full(k * ldbv, np.nan, dtype=dtype)
        for j in range(k):
            V[j * ldv:j * ldv + n] = draw(n) / np.sqrt(k)
            BV[j * ldbv:j * ldbv + n] = draw(n) / np.sqrt(k)
        coef = draw(k)
        w, bw = np.full(n + TAIL, 3.0, dtype=dtype), np.full(n + TAIL, 5.0, dtype=dtype)
        w[:n], bw[:n] = draw(n), draw(n)
        if n > 1:
            w[1] = -0.0
        A = K.arithmetic(cplx)
        scalars = [(float(c.real), float(c.imag)) for c in coef] if cplx else [float(c) for c in coef]
        with np.errstate(all="ignore"):
            rw, rbw, q = GK.update_pair([V[j * ldv:j * ldv + n] for j in range(k)], [BV[j * ldbv:j * ldbv + n] for j in range(k)],
                                        scalars, w[:n].copy(), bw[:n].copy(), A)
        want_w, want_bw = w.copy(), bw.copy()
        want_w[:n], want_bw[:n] = rw, rbw
        for a in (V, BV, coef, w, bw, want_w, want_bw):
            a.setflags(write=False)
        _cases[key] = (V, BV, coef, w, bw, want_w, want_bw, q, ldv, ldbv)
    return _cases[key]


def run(pkg, torch, n, k, cplx, with_q=True):
    """(w, bw, q, q of spl_vector_dot_dev on the results, V and BV as the call left them)"""
    V, BV, coef, w, bw, _, _, _, ldv, ldbv = case_of(n, k, cplx)
    lib = pkg._ffi.lib()
    dV, dBV, dc, dw, dbw = (dev(torch, a) for a in (V, BV, coef, w, bw))
    dq = dev(torch, np.array([7.0, 9.0]))
    ddot = dev(torch, np.array([7.0, 7.0]))
    stream = torch.cuda.current_stream().cuda_stream
    st = lib.spl_vector_update_pair_dev(n, 2 if cplx else 1, k, dV.data_ptr(), ldv, dBV.data_ptr(), ldbv, dc.data_ptr(),
                                        dw.data_ptr(), dbw.data_ptr(), dq.data_ptr() if with_q else None, stream)
    assert st == OK, st
    assert lib.spl_vector_dot_dev(n, 2 if cplx else 1, dw.data_ptr(), dbw.data_ptr(), ddot.data_ptr(), stream) == OK
    torch.cuda.synchronize()
    return dw.cpu().numpy(), dbw.cpu().numpy(), dq.cpu().numpy(), ddot.cpu().numpy(), dV.cpu().numpy(), dBV.cpu().numpy()


def nan_bits_equal(a, b):
    return K.bits_equal(np.nan_to_num(np.ascontiguousarray(a).view(np.float64), nan=5.0),
                        np.nan_to_num(np.ascontiguousarray(b).view(np.float64), nan=5.0))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n", SIZES)
def test_the_results_are_the_restatement_and_q_is_the_dot(gpu, pkg, n, cplx):
    for k in COLUMNS:
        V, BV, _, _, _, want_w, want_bw, want_q, _, _ = case_of(n, k, cplx)
        w, bw, q, dot, V_after, BV_after = run(pkg, gpu, n, k, cplx)
        assert K.bits_equal(w, want_w) and K.bits_equal(bw, want_bw), (n, k)  # rows from n on included
        assert nan_bits_equal(V_after, V) and nan_bits_equal(BV_after, BV)  # the columns, and the gaps between them
        assert K.bits_equal(q[:1], dot[:1]), (n, k, q, dot)  # the real part of the existing call's value
        assert K.bits_equal(q[:1], np.array([want_q])) and q[1] == 9.0  # one double is written
        if n == 0:
            assert K.bits_equal(q[:1], np.array([0.0]))  # +0.0
        w2, bw2, q2, _, _, _ = run(pkg, gpu, n, k, cplx, with_q=False)
        assert K.bits_equal(w2, want_w) and K.bits_equal(bw2, want_bw) and list(q2) == [7.0, 9.0]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_the_grid_does_not_show_in_the_bits(gpu, pkg, monkeypatch, cplx):
    n, k = 8209, 5
    _, _, _, _, _, want_w, want_bw, want_q, _, _ = case_of(n, k, cplx)
    for grid in ("1", "2", "7"):
        monkeypatch.setenv("SPL_KRYLOV_GRID", grid)
        w, bw, q, dot, _, _ = run(pkg, gpu, n, k, cplx)
        assert K.bits_equal(w, want_w) and K.bits_equal(bw, want_bw)
        assert K.bits_equal(q[:1], np.array([want_q])) and K.bits_equal(q[:1], dot[:1])


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_refusals_in_the_header_s_order(gpu, pkg, cplx):
    """every refused call but the last group breaks TWO rules: the one whose status is expected and one further down"""
    lib = pkg._ffi.lib()
    n, k, vw = 16, 3, 2 if cplx else 1
    entry = 8 * vw
    dtype = np.complex128 if cplx else np.float64
    block = dev(gpu, np.ones(8 * n, dtype=dtype))  # V: 3 columns; BV: 3 columns; w; bw
    base = block.data_ptr()
    good = dict(n=n, vw=vw, k=k, V=base, ldv=n, BV=base + 3 * n * entry, ldbv=n, coef=base, w=base + 6 * n * entry,
                bw=base + 7 * n * entry, q=None)

    def call(**change):
        a = dict(good, **change)
        st = lib.spl_vector_update_pair_dev(a["n"], a["vw"], a["k"], a["V"], a["ldv"], a["BV"], a["ldbv"], a["coef"], a["w"],
                                            a["bw"], a["q"], None)
        gpu.cuda.synchronize()
        return st

    ladder = [
        (dict(n=-1, vw=3), NEG),                      # n before the value width
        (dict(n=-1, V=None), NEG),
        (dict(vw=3, V=None), ARG),                    # the scalars before the pointers
        (dict(vw=0, w=None), ARG),
        (dict(k=0, BV=None), ARG),
        (dict(k=129, coef=None), ARG),
        (dict(ldv=n - 1, bw=None), ARG),
        (dict(ldbv=n - 1, w=good["w"] + entry // 2), ARG),
        (dict(V=None, w=good["w"] + entry // 2), ARG),    # the pointers before the alignment
        (dict(BV=None, bw=good["w"]), ARG),
        (dict(coef=None, bw=good["w"]), ARG),
        (dict(w=None, V=good["V"] + entry // 2), ARG),
        (dict(bw=None, V=good["V"] + entry // 2), ARG),
        (dict(V=good["V"] + entry // 2, bw=good["w"]), ARG),   # the alignment before the overlaps
        (dict(BV=good["BV"] + entry // 2, bw=good["w"]), ARG),
        (dict(coef=good["coef"] + entry // 2, bw=good["w"]), ARG),
        (dict(w=good["w"] + entry // 2), ARG),
        (dict(bw=good["bw"] + entry // 2), ARG),
        (dict(q=base + 4), ARG),
        (dict(bw=good["w"]), ARG),                             # w and bw over each other
        (dict(bw=good["w"] + (n - 1) * entry), ARG),
        (dict(w=good["V"] + (3 * n - 1) * entry), ARG),        # w over the last entry of V
        (dict(w=good["BV"]), ARG),
        (dict(bw=good["V"]), ARG),
        (dict(bw=good["BV"] + (3 * n - 1) * entry), ARG),
    ]
    for bad, status in ladder:
        assert call(**bad) == status, (bad, status)
    assert np.array_equal(block.cpu().numpy(), np.ones(8 * n, dtype=dtype))  # nothing was written
    assert call(n=0, V=None, BV=None, w=None, bw=None) == OK  # the vector pointers only when n > 0
    assert call(n=0, V=None, BV=None, w=None, bw=None, coef=None) == ARG
    assert call() == OK
