"""LU from device-resident matrix handles, the part that needs no GPU: the four entry points are declared in
include/umfpack_hip.h, exported by the library and bound by the Python mirror; without a device `analyzeDevice` /
`factorDevice` fail loudly with BackendUnavailable and never compute."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("spl_umfpack_di_symbolic_dev", "spl_umfpack_zi_symbolic_dev", "spl_umfpack_di_numeric_dev",
           "spl_umfpack_zi_numeric_dev")


def test_entry_points_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "umfpack_hip.h")).read()
    for name in SYMBOLS:
        args = "void *H, void **Symbolic" if "symbolic" in name else "void *H, void *Symbolic, void **Numeric"
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, re.escape(args)), text), name


def test_entry_points_are_exported_and_bound(pkg):
    import ctypes as C
    L = pkg.umfpack._declare()
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError: not exported
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == (2 if "symbolic" in name else 3)


class _NoMatrix(object):
    """stands where a DeviceMatrix would: any use of it is a computation that must not happen"""
    def __getattr__(self, name):
        raise AssertionError("touched the matrix (%s) without a device" % name)


def test_without_a_device_the_calls_fail_loudly(pkg):
    if pkg._ffi.device_count() > 0:
        return  # a device is visible: the loud failure is for machines without one
    with pytest.raises(pkg._ffi.BackendUnavailable):
        pkg.umfpack.analyzeDevice(_NoMatrix())
    with pytest.raises(pkg._ffi.BackendUnavailable):
        pkg.umfpack.factorDevice(_NoMatrix(), None)
    with pytest.raises(pkg._ffi.BackendUnavailable):
        pkg.DeviceMatrix.from_csc(pkg.ident(3))
