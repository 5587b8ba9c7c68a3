"""spl_vector_gram_dev and spl_vector_rotate_z_dev without a GPU: the restatements of tests/gram_cases.py checked on their
own (against krylov_cases.dot entry by entry, and against numpy to rounding level), the symbols and the Python surface,
and what the calls answer before the device is touched: every argument the header refuses is refused without a device,
and a negative length is refused before anything else.  The order AMONG the other refusals (width, ranges, NULL,
alignment, overlap) cannot be observed, because they all answer SPL_ERROR_argument_missing: it is not tested."""
import ctypes as C

import numpy as np
import pytest

import gram_cases as GK
import krylov_cases as K

EPS = 2.0 ** -53
SYMBOLS = {"spl_vector_gram_dev": 12, "spl_vector_rotate_z_dev": 11}
OK, MISSING, NONPOSITIVE = 0, -5, -6


def test_the_two_symbols_are_declared_exported_and_bound(pkg):
    """the header declares them, the library exports them and the binding knows their arguments"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sparse_linear_hip.h")).read()
    L = pkg._ffi.lib()
    for name, nargs in SYMBOLS.items():
        declared = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert declared and declared.group(1).count(",") + 1 == nargs, name
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes and len(fn.argtypes) == nargs, name
    assert pkg.vector_gram_dev is pkg.sparse.vector_gram_dev and callable(pkg.sparse.vector_rotate_dev)
    with pytest.raises(ValueError):
        pkg.sparse.vector_rotate_dev(4, 2, 1, 0, 4, 0, 2, Y_is_complex=True)  # a complex Y on real vectors


@pytest.mark.parametrize("length", [0, 1, 255, 257, 4096, 4097, 3 * 4096 + 5])
def test_fold_of_many_rows_is_the_fold_of_each(length):
    rng = np.random.default_rng(length)
    P = rng.standard_normal((5, length)) * 10.0 ** rng.integers(-6, 7, (5, length))
    got = GK.fold_many(P)
    assert K.bits_equal(got, np.array([K.fold(P[i]) for i in range(5)]))
    assert not np.signbit(GK.fold_many(np.zeros((2, length)))).any()  # +0.0


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n,k,l", [(0, 2, 3), (1, 1, 1), (257, 3, 2), (4097, 5, 4), (3 * 4096 + 5, 2, 3)])
def test_gram_is_the_single_inner_product_entry_by_entry(n, k, l, cplx):
    V, W = GK.blocks(n, k, l, cplx)
    G = GK.gram(V, W)
    want = np.array([[K.dot(V[:, i], W[:, j]) for j in range(l)] for i in range(k)], dtype=G.dtype).reshape(k, l)
    assert K.bits_equal(G, want)
    if n:
        # against numpy: |error| <= n 2^-53 sum |v_i| |w_i| per real sum, twice that for the four-product complex form
        bound = 4.0 * n * EPS * (np.abs(V).T @ np.abs(W)) + 1e-320
        assert (np.abs(G - V.conj().T @ W) <= bound).all()


def test_complex_rotation_is_the_product():
    rng = np.random.default_rng(5)
    V = rng.standard_normal((37, 9)) + 1j * rng.standard_normal((37, 9))
    Y = rng.standard_normal((9, 4)) + 1j * rng.standard_normal((9, 4))
    got = GK.rotate_z(V, Y)
    bound = 4.0 * 9 * EPS * (np.abs(V) @ np.abs(Y))
    assert got.dtype == np.complex128 and (np.abs(got - V @ Y) <= bound).all()
    # one term: Data.Complex's product, operation by operation
    a, b, c, d = Y[0, 0].real, Y[0, 0].imag, V[:, 0].real, V[:, 0].imag
    one = GK.rotate_z(V[:, :1], Y[:1, :1])[:, 0]
    assert K.bits_equal(one.real, a * c - b * d) and K.bits_equal(one.imag, a * d + b * c)
    # a real Y is the real rotation's result wherever no -0.0 * finite term changes a sign: here, to rounding level
    import eigsh_cases as EK
    assert np.allclose(GK.rotate_z(V, Y.real + 0j), EK.rotate(V, Y.real), rtol=1e-14, atol=1e-14)


def test_gram_refuses_before_the_device(pkg):
    L = pkg._ffi.lib()
    room = C.create_string_buffer(4096)
    at = (C.addressof(room) + 15) & ~15
    v, w, g = at, at + 1024, at + 2048

    def call(n=4, vw=1, k=2, l=2, V=v, ldv=4, W=w, ldw=4, G=g, ldg=2, upper=0):
        return L.spl_vector_gram_dev(n, vw, k, l, V, ldv, W, ldw, G, ldg, upper, None)

    assert call(n=-1, vw=3, k=0, G=None) == NONPOSITIVE  # the length comes first
    for bad in (dict(vw=0), dict(vw=3), dict(k=0), dict(k=129), dict(l=0), dict(l=129), dict(upper=2), dict(upper=-1),
                dict(ldv=3), dict(ldw=3), dict(ldg=1), dict(V=None), dict(W=None), dict(G=None),
                dict(n=0, V=None, W=None, G=None), dict(V=v + 4), dict(vw=2, V=v + 8), dict(vw=2, W=w + 8),
                dict(vw=2, G=g + 8), dict(G=v), dict(G=v + 8 * 7), dict(G=w + 8 * 7), dict(G=v - 8 * 3)):
        assert call(**bad) == MISSING, bad
    # the one order that shows: a negative length answers before a missing pointer
    assert call(n=-1, V=None) == NONPOSITIVE


def test_complex_rotation_refuses_before_the_device(pkg):
    L = pkg._ffi.lib()
    room = C.create_string_buffer(8192)
    at = (C.addressof(room) + 15) & ~15
    v, y, o = at, at + 2048, at + 4096

    def call(n=4, vw=2, m=2, k=1, V=v, ldv=8, Y=y, ldy=4, out=o, ldo=8):
        return L.spl_vector_rotate_z_dev(n, vw, m, k, V, ldv, Y, ldy, out, ldo, None)

    assert call(n=-1, vw=3) == NONPOSITIVE
    for bad in (dict(vw=1), dict(vw=0), dict(vw=3), dict(m=0), dict(m=129), dict(k=0), dict(k=3), dict(ldv=3), dict(ldy=1),
                dict(ldo=3), dict(V=None), dict(Y=None), dict(V=v + 8), dict(Y=y + 4), dict(out=o + 8), dict(out=v),
                dict(out=v + 16 * 11)):
        assert call(**bad) == MISSING, bad
