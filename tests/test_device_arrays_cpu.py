"""Compressed arrays and triples in device memory, in and out (spl_matrix_create_csr_dev, _create_csc_dev,
_compress_dev_wide, _export_csr_dev, _export_csc_dev; DeviceMatrix.from_torch / to_torch): what they answer before the
device is touched.  Argument checks come first and in a fixed order, so these hold with or without a GPU; no call here
passes a pointer the library would read."""
import ctypes as C

import pytest

SYMBOLS = ("spl_matrix_create_csr_dev", "spl_matrix_create_csc_dev", "spl_matrix_compress_dev_wide",
           "spl_matrix_export_csr_dev", "spl_matrix_export_csc_dev")
METHODS = ("from_csr_dev", "from_csc_dev", "compress_dev", "export_csr_dev", "export_csc_dev", "from_torch", "to_torch")


def _buffer():
    """64 bytes of host memory at an 8-byte aligned address: a stand-in for an array that is never read, because
    every call it is passed to is refused first"""
    raw = C.create_string_buffer(80)
    return raw, (C.addressof(raw) + 7) & ~7


def _imports(L):
    """the three imports as f(nrows, ncols, index_width, first_array, value_width, H), count 0 for the triples"""
    def csr(nr, nc, iw, p, vw, H):
        return L.spl_matrix_create_csr_dev(nr, nc, iw, p, None, None, vw, H)

    def csc(nr, nc, iw, p, vw, H):
        return L.spl_matrix_create_csc_dev(nr, nc, iw, p, None, None, vw, H)

    def coo(nr, nc, iw, p, vw, H):
        return L.spl_matrix_compress_dev_wide(nr, nc, 0, iw, p, p, None, vw, H, None)

    return (("csr", csr), ("csc", csc), ("coo", coo))


def test_the_five_symbols_and_the_methods_exist(pkg):
    L = pkg._ffi.lib()
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int and fn.argtypes, name
    for name in METHODS:
        assert callable(getattr(pkg.DeviceMatrix, name)), name


def test_imports_follow_the_status_ladder_in_its_order(pkg):
    F = pkg._ffi
    L = F.lib()
    keep, p = _buffer()
    for name, call in _imports(L):
        # 1. no output: nothing else is looked at
        assert call(-1, 1 << 31, 3, None, 7, None) == F.SPL_ERROR_argument_missing, name
        # the output is cleared whatever the call then answers
        h = C.c_void_p(0x1234)
        assert call(-1, 3, 4, p, 1, C.byref(h)) == F.SPL_ERROR_n_nonpositive and not h.value, name
        # 3. negative dimensions, before sizes and widths
        for nr, nc in ((-1, 3), (3, -1), (-1, 1 << 31)):
            h = C.c_void_p(0x1234)
            assert call(nr, nc, 3, None, 0, C.byref(h)) == F.SPL_ERROR_n_nonpositive and not h.value, name
        # 4. dimensions of 2^31, before widths and pointers
        for nr, nc in ((1 << 31, 3), (3, 1 << 31)):
            h = C.c_void_p(0x1234)
            assert call(nr, nc, 3, None, 0, C.byref(h)) == F.SPL_ERROR_index_overflow and not h.value, name
        # 5. widths, NULL and misaligned pointer arrays
        for iw in (0, 2, 3, 16):
            h = C.c_void_p(0x1234)
            assert call(3, 3, iw, p, 1, C.byref(h)) == F.SPL_ERROR_argument_missing and not h.value, (name, iw)
        for vw in (0, 3):
            h = C.c_void_p(0x1234)
            assert call(3, 3, 4, p, vw, C.byref(h)) == F.SPL_ERROR_argument_missing and not h.value, (name, vw)
        for iw in (4, 8):
            h = C.c_void_p(0x1234)
            assert call(3, 3, iw, p + 1, 1, C.byref(h)) == F.SPL_ERROR_argument_missing and not h.value, (name, iw)
        h = C.c_void_p(0x1234)
        assert call(3, 3, 8, p + 4, 1, C.byref(h)) == F.SPL_ERROR_argument_missing and not h.value, name  # 4-aligned, width 8
    # a NULL pointer array (the triples take none when there are no triples)
    for name, call in _imports(L)[:2]:
        h = C.c_void_p(0x1234)
        assert call(3, 3, 4, None, 1, C.byref(h)) == F.SPL_ERROR_argument_missing and not h.value, name
    # the triples: a negative count, and arrays missing when there are triples
    h = C.c_void_p(0x1234)
    assert L.spl_matrix_compress_dev_wide(3, 3, -1, 4, p, p, p, 1, C.byref(h), None) == F.SPL_ERROR_n_nonpositive
    assert not h.value
    for rows, cols, vals in ((None, p, p), (p, None, p), (p, p, None)):
        h = C.c_void_p(0x1234)
        st = L.spl_matrix_compress_dev_wide(3, 3, 2, 8, rows, cols, vals, 2, C.byref(h), None)
        assert st == F.SPL_ERROR_argument_missing and not h.value
    del keep


def test_exports_refuse_what_is_no_handle_first(pkg):
    F = pkg._ffi
    L = F.lib()
    junk = C.create_string_buffer(256)  # readable where a handle's magic would be, and none
    keep, p = _buffer()
    for fn in (L.spl_matrix_export_csr_dev, L.spl_matrix_export_csc_dev):
        for H in (None, junk):
            assert fn(H, 4, p, p, p) == F.SPL_ERROR_invalid_handle
            assert fn(H, 3, None, None, None) == F.SPL_ERROR_invalid_handle  # the handle is looked at before the rest
    del keep


def test_a_well_formed_call_needs_a_device(pkg):
    F = pkg._ffi
    L = F.lib()
    if F.device_count() > 0:
        # with a GPU only a call that passes no array may run here: no triples, a 3 x 3 matrix without entries
        h = C.c_void_p(0x1234)
        assert L.spl_matrix_compress_dev_wide(3, 3, 0, 8, None, None, None, 2, C.byref(h), None) == F.SPL_OK and h.value
        L.spl_matrix_free(C.byref(h))
        assert not h.value
        return
    keep, p = _buffer()
    for name, call in _imports(L):
        for iw in (4, 8):
            for vw in (1, 2):
                h = C.c_void_p(0x1234)
                assert call(3, 3, iw, p, vw, C.byref(h)) == F.SPL_ERROR_device and not h.value, (name, iw, vw)
    del keep


def test_from_torch_refuses_before_any_library_call(pkg, monkeypatch):
    import torch

    def no_library(*a, **k):
        raise AssertionError("from_torch reached the library")

    monkeypatch.setattr(pkg._ffi, "require_gpu", no_library)
    monkeypatch.setattr(pkg.sparse, "lib", no_library)
    crow = torch.tensor([0, 1, 2], dtype=torch.int64)
    col = torch.tensor([0, 1], dtype=torch.int64)
    DM = pkg.DeviceMatrix
    with pytest.raises(TypeError):  # float32: nothing is cast
        DM.from_torch(torch.sparse_csr_tensor(crow, col, torch.ones(2, dtype=torch.float32), size=(2, 2)))
    with pytest.raises(ValueError):  # a CPU tensor: nothing is moved
        DM.from_torch(torch.sparse_csr_tensor(crow, col, torch.ones(2, dtype=torch.float64), size=(2, 2)))
    batched = torch.sparse_csr_tensor(torch.stack([crow, crow]), torch.stack([col, col]),
                                      torch.ones(2, 2, dtype=torch.float64), size=(2, 2, 2))
    with pytest.raises(ValueError):
        DM.from_torch(batched)
    with pytest.raises(TypeError):  # strided
        DM.from_torch(torch.eye(2, dtype=torch.float64))
    with pytest.raises(TypeError):
        DM.from_torch([[1.0, 0.0], [0.0, 1.0]])
