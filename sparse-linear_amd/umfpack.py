"""Mirror of ``Numeric.LinearAlgebra.Umfpack`` (suitesparse/src/Numeric/LinearAlgebra/Umfpack.hs).

Same interface as the reference: the simple ``linearSolve`` / ``solve`` (``<\\>``) and the
advanced ``analyze`` / ``factor`` / ``linearSolve_`` with ``UmfpackNormal`` / ``UmfpackTrans``,
over the same six ``umfpack_di_*`` C symbols (include/umfpack_hip.h) that the reference
imports (Umfpack/Internal.hs:137-148).  Handles are owned like the reference's ForeignPtrs:
the free function is the finalizer and receives a ``void**``.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import as_f64, lib, p_f64, p_i32

UmfpackNormal = 0  # sys = UMFPACK_A   (Umfpack.hs:95-97)
UmfpackTrans = 1   # sys = UMFPACK_At


class UmfpackError(RuntimeError):
    """negative status: the reference calls errorWithStackTrace (Umfpack.hs:67,81,101)"""

    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status  # the UMFPACK status behind it (None: raised by a check of this mirror)


def _declare():
    L = lib()
    if getattr(L, "_umf_declared", False):
        return L
    i, vp, ip, dp = C.c_int, C.c_void_p, _ffi.c_int_p, _ffi.c_dbl_p
    L.umfpack_di_symbolic.restype = i
    L.umfpack_di_symbolic.argtypes = [i, i, ip, ip, dp, C.POINTER(vp), dp, dp]
    L.umfpack_di_numeric.restype = i
    L.umfpack_di_numeric.argtypes = [ip, ip, dp, vp, C.POINTER(vp), dp, dp]
    L.umfpack_di_solve.restype = i
    L.umfpack_di_solve.argtypes = [i, ip, ip, dp, dp, dp, vp, dp, dp]
    L.umfpack_di_free_symbolic.restype = None
    L.umfpack_di_free_symbolic.argtypes = [C.POINTER(vp)]
    L.umfpack_di_free_numeric.restype = None
    L.umfpack_di_free_numeric.argtypes = [C.POINTER(vp)]
    L.umfpack_di_report_status.restype = None
    L.umfpack_di_report_status.argtypes = [dp, i]
    # instance Umfpack (Complex Double) (Umfpack/Internal.hs:117-135): packed mode, Az = Xz = Bz = NULL
    L.umfpack_zi_symbolic.restype = i
    L.umfpack_zi_symbolic.argtypes = [i, i, ip, ip, dp, dp, C.POINTER(vp), dp, dp]
    L.umfpack_zi_numeric.restype = i
    L.umfpack_zi_numeric.argtypes = [ip, ip, dp, dp, vp, C.POINTER(vp), dp, dp]
    L.umfpack_zi_solve.restype = i
    L.umfpack_zi_solve.argtypes = [i, ip, ip, dp, dp, dp, dp, dp, dp, vp, dp, dp]
    L.umfpack_zi_free_symbolic.restype = None
    L.umfpack_zi_free_symbolic.argtypes = [C.POINTER(vp)]
    L.umfpack_zi_free_numeric.restype = None
    L.umfpack_zi_free_numeric.argtypes = [C.POINTER(vp)]
    L.umfpack_zi_report_status.restype = None
    L.umfpack_zi_report_status.argtypes = [dp, i]
    L.spl_umfpack_di_solve_many.restype = i
    L.spl_umfpack_di_solve_many.argtypes = [i, ip, ip, dp, i, dp, dp, vp]
    L.spl_umfpack_zi_solve_many.restype = i
    L.spl_umfpack_zi_solve_many.argtypes = [i, ip, ip, dp, dp, i, dp, dp, dp, dp, vp]
    L.spl_umfpack_di_solve_many_dev.restype = i
    L.spl_umfpack_di_solve_many_dev.argtypes = [i, ip, ip, dp, i, vp, vp, vp]
    L.spl_umfpack_zi_solve_many_dev.restype = i
    L.spl_umfpack_zi_solve_many_dev.argtypes = [i, ip, ip, dp, i, vp, vp, vp]
    for name in ("spl_umfpack_di_symbolic_dev", "spl_umfpack_zi_symbolic_dev"):
        getattr(L, name).restype = i
        getattr(L, name).argtypes = [vp, C.POINTER(vp)]
    for name in ("spl_umfpack_di_numeric_dev", "spl_umfpack_zi_numeric_dev"):
        getattr(L, name).restype = i
        getattr(L, name).argtypes = [vp, vp, C.POINTER(vp)]
    L.spl_umfpack_dimension.restype = i
    L.spl_umfpack_dimension.argtypes = [vp]
    L.spl_umfpack_path.restype = i
    L.spl_umfpack_path.argtypes = [vp]
    L.spl_umfpack_stats.restype = C.c_int
    L.spl_umfpack_stats.argtypes = [vp, C.POINTER(C.c_double)]
    L.spl_umfpack_solve_report.restype = C.c_int
    L.spl_umfpack_solve_report.argtypes = [vp, C.POINTER(C.c_double)]
    L.umfpack_di_get_determinant.restype = i
    L.umfpack_di_get_determinant.argtypes = [dp, dp, vp, dp]
    L.spl_umfpack_di_log_determinant.restype = i
    L.spl_umfpack_di_log_determinant.argtypes = [vp, dp, dp]
    L.spl_umfpack_inertia.restype = i
    L.spl_umfpack_inertia.argtypes = [vp, dp]
    L.spl_umfpack_di_condest.restype = i
    L.spl_umfpack_di_condest.argtypes = [i, i, ip, ip, dp, vp, dp, dp]
    L.spl_umfpack_zi_condest.restype = i
    L.spl_umfpack_zi_condest.argtypes = [i, i, ip, ip, dp, dp, vp, dp, dp, dp]
    L._umf_declared = True
    return L


def _report(where, status):
    L = _declare()
    L.umfpack_di_report_status(None, status)  # umfpack_report_status mat nullPtr _stat
    if status < 0:
        raise UmfpackError("%s failed (status %d)" % (where, status), status)
    return status


class _Handle(_ffi.Handle):
    def __init__(self, value, free_name):
        _ffi.Handle.__init__(self, free_name, value)

    @property
    def value(self):  # not checked: a NULL object comes back as the call's own status
        return self._h


class Analysis(_Handle):
    """newtype Analysis a = Analysis { fsym :: ForeignPtr (Symbolic a) } (Umfpack.hs:56)"""
    complex = False


class Factors(_Handle):
    """newtype Factors a = Factors { fnum :: ForeignPtr (Numeric a) } (Umfpack.hs:58)"""
    status = 0
    complex = False

    @property
    def path(self):
        """factorisation held now: 0 band with partial pivoting, 1 band without interchanges
        (diagonally dominant), 2 the same as a speculation that every solve checks, 3 / 4
        multifrontal without interchanges (dominant / speculation), 5 multifrontal with static pivoting
        (maximum-product transversal + scalings, csrc/static_pivot.hpp) (include/umfpack_hip.h)"""
        return int(_declare().spl_umfpack_path(self.value))

    @property
    def stats(self):
        """figures of the factorisation held now (spl_umfpack_stats, include/umfpack_hip.h)"""
        buf = (C.c_double * 8)()
        if _declare().spl_umfpack_stats(self.value, buf) != 0:
            raise UmfpackError("spl_umfpack_stats: invalid Numeric object")
        keys = ("path", "n", "kl", "ku", "device_bytes", "flops", "fronts", "flags")
        st = dict(zip(keys, [float(v) if k in ("device_bytes", "flops") else int(v) for k, v in zip(keys, buf)]))
        flags = st.pop("flags")
        st["complex_fronts"] = flags & 1          # native complex fronts (zi objects)
        st["block_pivoting"] = (flags >> 1) & 1   # threshold pivoting inside the diagonal blocks of the fronts
        return st

    @property
    def determinant(self):
        """(mantissa, exponent10) of det A (module function `determinant`)"""
        return determinant(self)

    @property
    def logDeterminant(self):
        """(sign, ln |det A|) (module function `logDeterminant`)"""
        return logDeterminant(self)

    @property
    def inertia(self):
        """(positive, negative, zero) eigenvalue counts (module function `inertia`)"""
        return inertia(self)

    @property
    def solve_report(self):
        """the most recent solve on these factors and the bytes one walk over them reads (spl_umfpack_solve_report,
        include/umfpack_hip.h): what UMFPACK returns in Info[UMFPACK_IR_TAKEN / _IR_ATTEMPTED / _OMEGA1]"""
        buf = (C.c_double * 8)()
        if _declare().spl_umfpack_solve_report(self.value, buf) != 0:
            raise UmfpackError("spl_umfpack_solve_report: invalid Numeric object")
        return {"walks": int(buf[0]), "ir_taken": int(buf[1]), "ir_attempted": int(buf[2]),
                "backward_error": float(buf[3]), "walk_bytes": float(buf[4]),
                "chain_bytes": float(buf[5]), "chain_build_ms": float(buf[6]), "chain_span": int(buf[7])}


def analyze(mat):
    """symbolic analysis (Umfpack.hs:60-69)"""
    L = _declare()
    nr, nc, ap, ai, ax = mat._tuple32()
    sym = C.c_void_p()
    if mat.is_complex:
        st = L.umfpack_zi_symbolic(nr, nc, p_i32(ap), p_i32(ai), p_f64(ax), None, C.byref(sym), None, None)
        a = Analysis(sym.value, "umfpack_zi_free_symbolic")
        a.complex = True
        _report("analyze: umfpack_symbolic", st)
        return a
    st = L.umfpack_di_symbolic(nr, nc, p_i32(ap), p_i32(ai), p_f64(ax), C.byref(sym), None, None)
    a = Analysis(sym.value, "umfpack_di_free_symbolic")
    _report("analyze: umfpack_symbolic", st)
    return a


def factor(mat, analysis):
    """numeric factorisation (Umfpack.hs:71-83); needs a GPU"""
    L = _declare()
    _ffi.require_gpu()
    nr, nc, ap, ai, ax = mat._tuple32()
    num = C.c_void_p()
    if mat.is_complex:
        st = L.umfpack_zi_numeric(p_i32(ap), p_i32(ai), p_f64(ax), None, analysis.value, C.byref(num), None, None)
        f = Factors(num.value, "umfpack_zi_free_numeric")
        f.complex = True
        f.status = _report("factor: umfpack_numeric", st)
        return f
    st = L.umfpack_di_numeric(p_i32(ap), p_i32(ai), p_f64(ax), analysis.value, C.byref(num), None, None)
    f = Factors(num.value, "umfpack_di_free_numeric")
    f.status = _report("factor: umfpack_numeric", st)
    return f


def analyzeDevice(dm):
    """`analyze` of a device-resident matrix (a `DeviceMatrix`, real or complex): spl_umfpack_{di,zi}_symbolic_dev.
    The pattern crosses to the host once (the analysis is host code); the result serves `factor` and `factorDevice`."""
    L = _declare()
    _ffi.require_gpu()
    sym = C.c_void_p()
    if dm.is_complex:
        st = L.spl_umfpack_zi_symbolic_dev(dm.handle, C.byref(sym))
        a = Analysis(sym.value, "umfpack_zi_free_symbolic")
        a.complex = True
    else:
        st = L.spl_umfpack_di_symbolic_dev(dm.handle, C.byref(sym))
        a = Analysis(sym.value, "umfpack_di_free_symbolic")
    _report("analyzeDevice: umfpack_symbolic", st)
    return a


def factorDevice(dm, analysis):
    """`factor` of a device-resident matrix (spl_umfpack_{di,zi}_numeric_dev): the matrix is factored where it lies —
    nothing of it crosses PCIe, the embedding of a complex matrix is built by a kernel — and the handle is only
    borrowed: the factors keep their own device copies.  `analysis` may come from `analyze` or `analyzeDevice`."""
    L = _declare()
    _ffi.require_gpu()
    num = C.c_void_p()
    if dm.is_complex:
        st = L.spl_umfpack_zi_numeric_dev(dm.handle, analysis.value, C.byref(num))
        f = Factors(num.value, "umfpack_zi_free_numeric")
        f.complex = True
    else:
        st = L.spl_umfpack_di_numeric_dev(dm.handle, analysis.value, C.byref(num))
        f = Factors(num.value, "umfpack_di_free_numeric")
    f.status = _report("factorDevice: umfpack_numeric", st)
    return f


def linearSolve_(fact, mode, mat, b):
    """solve with existing factors (Umfpack.hs:87-102); returns the solution vector"""
    L = _declare()
    nr, nc, ap, ai, ax = mat._tuple32()
    # the C side copies nrows (2 nrows) doubles out of b: a short vector would be a heap over-read, and real
    # factors with a complex matrix (or the reverse) would be read with the wrong dimension
    if np.shape(b) != (mat.nrows,):
        raise UmfpackError("linearSolve_: right-hand side has shape %s, the matrix has %d rows" % (np.shape(b), mat.nrows))
    if bool(fact.complex) != bool(mat.is_complex):
        raise UmfpackError("linearSolve_: %s factors used with a %s matrix"
                           % ("complex" if fact.complex else "real", "complex" if mat.is_complex else "real"))
    if mat.is_complex:
        b = np.ascontiguousarray(b, dtype=np.complex128)
        soln = np.zeros(mat.ncols, dtype=np.complex128)
        st = L.umfpack_zi_solve(int(mode), p_i32(ap), p_i32(ai), p_f64(ax), None, p_f64(soln.view(np.float64)), None,
                                p_f64(b.view(np.float64)), None, fact.value, None, None)
        _report("linearSolve_: umfpack_solve", st)
        return soln
    b = as_f64(b)
    soln = np.zeros(mat.ncols, dtype=np.float64)  # MV.replicate ncols 0 (:93)
    st = L.umfpack_di_solve(int(mode), p_i32(ap), p_i32(ai), p_f64(ax), p_f64(soln), p_f64(b), fact.value,
                            None, None)
    _report("linearSolve_: umfpack_solve", st)
    return soln


def linearSolveMany_(fact, mode, mat, bs):
    """`map (linearSolve_ fact mode mat) bs` (Umfpack.hs:103-108) in ONE pass of all right-hand
    sides through the factors (spl_umfpack_{di,zi}_solve_many); returns the list of solutions"""
    L = _declare()
    bs = list(bs)
    k = len(bs)
    if k == 0:
        return []
    nr, nc, ap, ai, ax = mat._tuple32()
    if bool(fact.complex) != bool(mat.is_complex):
        raise UmfpackError("linearSolveMany_: %s factors used with a %s matrix"
                           % ("complex" if fact.complex else "real", "complex" if mat.is_complex else "real"))
    dt = np.complex128 if mat.is_complex else np.float64
    B = np.empty((k, mat.nrows), dtype=dt)  # row c = right-hand side c: column-major n x k for the C side
    for c, b in enumerate(bs):
        b = np.asarray(b)
        if b.shape != (mat.nrows,):
            raise UmfpackError("linearSolveMany_: right-hand side %d has shape %s" % (c, b.shape))
        B[c] = b
    X = np.zeros((k, mat.ncols), dtype=dt)
    if mat.is_complex:
        st = L.spl_umfpack_zi_solve_many(int(mode), p_i32(ap), p_i32(ai), p_f64(ax), None, k,
                                         p_f64(X.view(np.float64)), None, p_f64(B.view(np.float64)), None,
                                         fact.value)
    else:
        st = L.spl_umfpack_di_solve_many(int(mode), p_i32(ap), p_i32(ai), p_f64(ax), k, p_f64(X), p_f64(B),
                                         fact.value)
    _report("linearSolveMany_: umfpack_solve", st)
    return [X[c] for c in range(k)]


def linearSolve(mat, bs):
    """factor once, solve for every right-hand side (Umfpack.hs:38-46)"""
    fact = factor(mat, analyze(mat))
    return linearSolveMany_(fact, UmfpackNormal, mat, bs)


def solve(mat, b):
    """the reference's (<\\>) (Umfpack.hs:48-50)"""
    return linearSolve(mat, [b])[0]


def linearSolveManyDevice_(fact, mode, mat, B):
    """`linearSolveMany_` with the right-hand sides and the solutions in device memory: B is a torch tensor on
    the GPU of shape (k, nrows) — row c = right-hand side c, float64 for real factors, complex128 for complex
    ones — and the result is a new tensor of the same shape and device (spl_umfpack_{di,zi}_solve_many_dev).
    `mat` is the host `Matrix`, or a `DeviceMatrix` or None for factors of a device-resident matrix (`factorDevice`):
    the C side then gets NULL arrays, as umfpack_hip.h allows — the factors hold their own copy of the matrix."""
    import torch
    L = _declare()
    from .sparse import DeviceMatrix, Matrix
    if mat is None or isinstance(mat, DeviceMatrix):
        return _solve_many_device_null(L, fact, mode, mat, B)
    if not isinstance(mat, Matrix):
        raise UmfpackError("linearSolveManyDevice_: mat must be a Matrix, a DeviceMatrix or None, not %s" % type(mat).__name__)
    want = torch.complex128 if mat.is_complex else torch.float64
    if bool(fact.complex) != bool(mat.is_complex):
        raise UmfpackError("linearSolveManyDevice_: %s factors used with a %s matrix"
                           % ("complex" if fact.complex else "real", "complex" if mat.is_complex else "real"))
    if not (isinstance(B, torch.Tensor) and B.is_cuda and B.dtype == want and B.dim() == 2 and B.shape[1] == mat.nrows
            and B.is_contiguous()):
        raise UmfpackError("linearSolveManyDevice_: B must be a contiguous %s GPU tensor of shape (k, %d)" % (want, mat.nrows))
    k = int(B.shape[0])
    X = torch.zeros((k, mat.ncols), dtype=want, device=B.device)
    if k == 0:
        return X
    nr, nc, ap, ai, ax = mat._tuple32()
    torch.cuda.current_stream(B.device).synchronize()  # the library works on the null stream of the device
    fn = L.spl_umfpack_zi_solve_many_dev if mat.is_complex else L.spl_umfpack_di_solve_many_dev
    with torch.cuda.device(B.device):
        st = fn(int(mode), p_i32(ap), p_i32(ai), p_f64(ax), k, C.c_void_p(X.data_ptr()), C.c_void_p(B.data_ptr()), fact.value)
    _report("linearSolveManyDevice_: umfpack_solve", st)
    return X

def _solve_many_device_null(L, fact, mode, dm, B):
    """linearSolveManyDevice_ without host arrays: dm is a DeviceMatrix (checked against the factors) or None"""
    import torch
    n = int(L.spl_umfpack_dimension(fact.value)) // (2 if fact.complex else 1)
    if dm is not None:
        inf = dm.info()
        if bool(fact.complex) != bool(dm.is_complex):
            raise UmfpackError("linearSolveManyDevice_: %s factors used with a %s matrix"
                               % ("complex" if fact.complex else "real", "complex" if dm.is_complex else "real"))
        if inf["nrows_global"] != n or inf["ncols"] != n:
            raise UmfpackError("linearSolveManyDevice_: factors of %d unknowns used with a %d x %d matrix"
                               % (n, inf["nrows_global"], inf["ncols"]))
    want = torch.complex128 if fact.complex else torch.float64
    if not (isinstance(B, torch.Tensor) and B.is_cuda and B.dtype == want and B.dim() == 2 and B.shape[1] == n
            and B.is_contiguous()):
        raise UmfpackError("linearSolveManyDevice_: B must be a contiguous %s GPU tensor of shape (k, %d)" % (want, n))
    k = int(B.shape[0])
    X = torch.zeros((k, n), dtype=want, device=B.device)
    if k == 0:
        return X
    torch.cuda.current_stream(B.device).synchronize()  # the library works on the null stream of the device
    fn = L.spl_umfpack_zi_solve_many_dev if fact.complex else L.spl_umfpack_di_solve_many_dev
    with torch.cuda.device(B.device):
        st = fn(int(mode), None, None, None, k, C.c_void_p(X.data_ptr()), C.c_void_p(B.data_ptr()), fact.value)
    _report("linearSolveManyDevice_: umfpack_solve", st)
    return X


_PATH_NAMES = {0: "band LU with partial pivoting", 1: "band without interchanges", 2: "band without interchanges (speculation)",
               3: "multifrontal without interchanges", 4: "multifrontal without interchanges (speculation)",
               5: "multifrontal with static pivoting"}


def _real_factors(fact, what):
    if fact.complex:
        raise UmfpackError("%s: complex factors are not served — where the native complex fronts are not used they are "
                           "the factors of the real 2n embedding, whose determinant is |det A|^2 and has lost the phase"
                           % what)


def determinant(fact):
    """det A = mantissa * 10**exponent10 with 1 <= |mantissa| < 10 (0, 0 when singular), from the factors
    (umfpack_di_get_determinant); factors that are still a speculation are checked first, as a solve checks them"""
    _real_factors(fact, "determinant")
    mx, ex = C.c_double(), C.c_double()
    _report("determinant: umfpack_di_get_determinant",
            _declare().umfpack_di_get_determinant(C.byref(mx), C.byref(ex), fact.value, None))
    return mx.value, int(ex.value)


def logDeterminant(fact):
    """(sign, ln |det A|) with sign in {-1, 0, 1} (ln|det| = -inf when singular): numpy's slogdet, never overflows
    (spl_umfpack_di_log_determinant)"""
    _real_factors(fact, "logDeterminant")
    sg, la = C.c_double(), C.c_double()
    _report("logDeterminant: spl_umfpack_di_log_determinant",
            _declare().spl_umfpack_di_log_determinant(fact.value, C.byref(sg), C.byref(la)))
    return int(sg.value), la.value


def inertia(fact):
    """(positive, negative, zero) eigenvalue counts of a symmetric A (spl_umfpack_inertia) — only when the factors held
    are a congruence of A (no interchanges, no scaling); raises UmfpackError naming what prevents it otherwise"""
    _real_factors(fact, "inertia")
    out = (C.c_double * 3)()
    st = _declare().spl_umfpack_inertia(fact.value, out)
    if st == -13:  # UMFPACK_ERROR_invalid_system: not a congruence of A
        path = fact.path
        why = _PATH_NAMES.get(path, "path %d" % path)
        if path in (1, 2, 3, 4):
            why += ", with threshold pivoting inside the diagonal blocks" if fact.stats["block_pivoting"] else \
                ", of a matrix that is not symmetric (or singular)"
        raise UmfpackError("inertia: the factors held (path %d: %s) are not a congruence of A" % (path, why), st)
    _report("inertia: spl_umfpack_inertia", st)
    return int(out[0]), int(out[1]), int(out[2])


def det(mat):
    """determinant of a real square matrix: analyse, factor, read the pivots; returns (mantissa, exponent10)"""
    return determinant(factor(mat, analyze(mat)))


def slogdet(mat):
    """(sign, ln |det A|) of a real square matrix: analyse, factor, read the pivots"""
    return logDeterminant(factor(mat, analyze(mat)))


def conditionEstimate(fact, mat, norm=1, t=2):
    """kappa_1(A) (norm=1) or kappa_inf(A) (norm=np.inf) from the factors, on the device (spl_umfpack_{di,zi}_condest):
    ||A|| exact, ||A^-1|| by Higham & Tisseur's block 1-norm estimator with t columns — a lower bound, in practice exact
    or within a factor of 3.  Returns {cond, norm_A, norm_inv, iterations, solves, witness}: the witness x proves the
    estimate, ||A^-1 x|| >= norm_inv ||x|| in the chosen norm (equal for norm=1)."""
    L = _declare()
    if bool(fact.complex) != bool(mat.is_complex):
        raise UmfpackError("conditionEstimate: %s factors used with a %s matrix"
                           % ("complex" if fact.complex else "real", "complex" if mat.is_complex else "real"))
    if norm == 1:
        sys = UmfpackNormal
    elif norm == np.inf:
        sys = UmfpackTrans  # kappa_1(A^T) = kappa_inf(A); A^H for complex factors, the same figure
    else:
        raise UmfpackError("conditionEstimate: norm must be 1 or numpy.inf, not %r" % (norm,))
    nr, nc, ap, ai, ax = mat._tuple32()
    out = (C.c_double * 6)()
    if mat.is_complex:
        x = np.zeros(mat.ncols, dtype=np.complex128)
        st = L.spl_umfpack_zi_condest(sys, int(t), p_i32(ap), p_i32(ai), p_f64(ax), None, fact.value, out,
                                      p_f64(x.view(np.float64)), None)
    else:
        x = np.zeros(mat.ncols, dtype=np.float64)
        st = L.spl_umfpack_di_condest(sys, int(t), p_i32(ap), p_i32(ai), p_f64(ax), fact.value, out, p_f64(x))
    _report("conditionEstimate: spl_umfpack_condest", st)
    return {"cond": out[0], "norm_A": out[1], "norm_inv": out[2], "iterations": int(out[3]), "solves": int(out[4]),
            "t": int(out[5]), "witness": x if st == 0 else None}


def condest(mat, norm=1):
    """condition number estimate of a square matrix in the 1-norm (or numpy.inf): analyse, factor, estimate"""
    return conditionEstimate(factor(mat, analyze(mat)), mat, norm)["cond"]
