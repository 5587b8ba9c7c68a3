"""Host-side mirror of ``Data.Matrix.Sparse`` (sparse-linear/src/Data/Matrix/Sparse.hs).

Same names, argument order, meaning and error behaviour as the reference's
export list (Sparse.hs:13-30), so code and tests written against the Haskell
API read the same here.  ``Matrix`` is the reference's CSC record
(Sparse.hs:67-76) with 64-bit ``pointers`` / ``indices`` and fp64 ``values``.

Everything on the hot path — ``mulV``, ``axpy``, ``axpy_``, ``mulM``, ``mm`` /
``*``, ``lin`` / ``+`` / ``-``, ``transpose``, ``compress`` / ``fromTriples`` —
crosses the C ABI (include/sparse_linear_hip.h) into the gfx950 kernels, with
the int64 -> int32 narrowing of ``withConstMatrix`` (Foreign.hs:39-41) at the
seam.  There is no CPU implementation of those operations in this package: if
the shared library or a GPU is missing they raise.

The purely structural combinators (``hcat``, ``vcat``, ``fromBlocks*``,
``kronecker``, ``diag``, ``ident``, ``zeros``, ``takeDiag``, ``pack`` …) only
rearrange index arrays; they are host-side numpy here (SURVEY.md §8f rank 4
lists their device versions as "next").  ``DeviceMatrix`` has them handle to
handle (``kronecker``, ``assemble`` / ``hcat`` / ``vcat`` / ``from_blocks*`` /
``block_diag``, ``take_diag``, ``diag_dev`` / ``ident``): nothing crosses PCIe.  CSR / CSC / COO arrays that already
lie in device memory, a sparse torch tensor on the GPU among them, enter and leave a handle the same way
(``from_csr_dev``, ``from_csc_dev``, ``compress_dev``, ``export_csr_dev``, ``export_csc_dev``, ``from_torch``,
``to_torch``).  A handle is taken apart the same way: ``submatrix`` / ``A[a:b, c:d]`` for a window, ``select`` /
``A[rows, cols]`` for rows and columns by index (a permutation ``P A Q`` among them); ``subMatrix`` is the host route.
Its values are worked on entry by entry the same way: ``map`` / ``negate`` / ``abs`` / ``signum`` / ``conj`` / ``real`` /
``imag`` / ``scale``, ``scale_rows_cols``, ``drop_zeros`` / ``drop_small``, ``band`` / ``tril`` / ``triu``, ``abs_sums`` /
``abs_max`` / ``norm``; the host ``cmap`` and ``scale`` below stay numpy.  Systems with a handle's lower or upper triangle
are solved on the device by ``DeviceMatrix.triangular`` / ``TriangularSolver`` (``solveTriangular`` from a host Matrix),
and ``DeviceMatrix.ilu0`` / ``ILU0`` (``ilu0`` from a host Matrix) produces the incomplete factors those solvers apply.
``DeviceMatrix.krylov`` / ``KrylovSolver`` (``cg`` / ``bicgstab`` from a host Matrix) solve ``A x = b`` with them:
preconditioned CG and BiCGSTAB whose scalars stay on the device; ``vector_dot_dev`` is their fixed-order inner product.
``DeviceMatrix.gmres`` / ``GMRESSolver`` (``gmres`` from a host Matrix) is restarted GMRES for unsymmetric and indefinite
systems with the same preconditioners; ``vector_dots_dev`` is the k-column inner product its orthogonalisation uses,
and ``vector_gram_dev`` the k x l block of inner products of two column blocks in one pass.
``DeviceMatrix.lobpcg`` / ``LOBPCGSolver`` (``lobpcg`` from a host Matrix) is the block eigensolver; with ``B=`` (or
``LOBPCGSolver.set_mass``) it solves ``A x = lambda B x`` for a Hermitian positive definite mass matrix, and
``vector_update_pair_dev`` is the paired update of a column and its image under ``B`` that its orthogonalisation uses.
``DeviceMatrix.amg`` / ``AMG`` (``amg`` from a host Matrix) build an aggregation multigrid hierarchy from the handle
operations above, and its V-cycle is a preconditioner the solvers take (``M=<AMG>`` or ``M="amg"``).
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import (SPL_ERROR_dimension_mismatch, SPL_ERROR_index_out_of_bounds, as_f64, as_i32, check,
                   lib, p_f64, p_i32)

I64 = np.int64
F64 = np.float64
C128 = np.complex128


class SparseError(ValueError):
    """The reference's ``errorWithStackTrace`` / ``error`` call sites."""


def _oops(fn, msg):
    raise SparseError("%s: %s" % (fn, msg))


def _vector_arg(where, v, shape, cplx, what, the=None, tensor=None):
    """The vector or block argument v of `where`: a torch tensor on the device or what numpy reads (tensor True / False:
    which of the two it has to be; None: as v is), of the shape `shape`, (n,) or (n, k), complex128 when cplx and
    float64 otherwise.  what / the: its name in the refusal of an array ("a start") and of a tensor ("start"; None: the
    only argument).  Returns (v or the array, the dtype wanted, is a tensor)"""
    size = " x ".join("%d" % d for d in shape)
    if tensor is None:
        try:
            import torch
            tensor = isinstance(v, torch.Tensor)
        except ImportError:  # pragma: no cover
            tensor = False
    if tensor:
        import torch
        want = torch.complex128 if cplx else torch.float64
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == want and tuple(v.shape) == tuple(shape)):
            needed = "a device tensor of %s %s entries" % (size, want)
            _oops(where, "the %s must be %s" % (the, needed) if the else needed + " is needed")
        return v, want, True
    want = C128 if cplx else F64
    a = np.atleast_1d(np.asarray(v))  # a scalar is a vector of one entry
    if a.dtype != want or a.shape != tuple(shape):
        _oops(where, "%s of dtype %s and shape %s; %s %s entries are needed"
              % (what, a.dtype, a.shape, size, np.dtype(want)))
    return a, want, False


def _frozen(a):
    """a read-only view of `a` (the caller's own array object keeps its flags); an array that is read-only already —
    the field of another Matrix — is passed on as the object it is, so matrices built from the same pattern share it"""
    if not a.flags.writeable:
        return a
    v = a.view()
    v.setflags(write=False)
    return v


def _sample(a, k=2048):
    n = len(a)
    if n <= k:
        return a.copy()
    return a[np.linspace(0, n - 1, k).astype(np.int64)]


def _pattern_fingerprint(pointers, indices):
    return (len(pointers), len(indices), _sample(pointers), _sample(indices))


def _same_fingerprint(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


class Matrix(object):
    """Matrix in compressed sparse column (CSC) format (Sparse.hs:67-76)."""

    __slots__ = ("ncols", "nrows", "pointers", "indices", "values", "_handle", "_narrowed", "__weakref__")

    def __init__(self, ncols, nrows, pointers, indices, values):
        self.ncols = int(ncols)
        self.nrows = int(nrows)
        # read-only views: a Matrix is a value (the fields of the Haskell record cannot change), and the FFI seam keeps
        # narrowed copies of the pattern (_tuple32) — an in-place edit through the Matrix raises instead of going unnoticed
        self.pointers = _frozen(np.ascontiguousarray(pointers, dtype=I64))
        self.indices = _frozen(np.ascontiguousarray(indices, dtype=I64))
        values = np.asarray(values)
        # Double, or Complex Double (the reference's two SPECIALIZE instances, Sparse.hs:456-457)
        self.values = np.ascontiguousarray(values, dtype=C128 if np.iscomplexobj(values) else F64)
        self._handle = None

    @property
    def is_complex(self):
        return self.values.dtype == C128

    # deriving Eq (Sparse.hs:78): structural equality, explicit zeros included
    def __eq__(self, other):
        if not isinstance(other, Matrix):
            return NotImplemented
        return (self.ncols == other.ncols and self.nrows == other.nrows
                and np.array_equal(self.pointers, other.pointers)
                and np.array_equal(self.indices, other.indices)
                and np.array_equal(self.values, other.values))

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    __hash__ = None

    def __repr__(self):
        return "Matrix {ncols = %d, nrows = %d, pointers = %s, indices = %s, values = %s}" % (
            self.ncols, self.nrows, self.pointers.tolist(), self.indices.tolist(), self.values.tolist())

    # instance Num (Sparse.hs:100-113)
    def __add__(self, other):
        return lin(1.0, self, 1.0, other)  # glin 0 (+) a (+) b

    def __sub__(self, other):
        return lin(1.0, self, -1.0, other)  # glin 0 (+) a (-) b

    def __mul__(self, other):
        return mm(self, other)

    def __neg__(self):
        return cmap(np.negative, self)

    def __abs__(self):
        return cmap(np.abs, self)

    def signum(self):
        return cmap(np.sign, self)

    # -- FFI seam -----------------------------------------------------------------------
    def _tuple32(self):
        """withConstMatrix's marshalling (Foreign.hs:24-41): fresh int32 copies.  Complex values
        cross as packed (re, im) pairs, the form the reference passes to umfpack_zi_* with the
        imaginary pointer NULL (Umfpack/Internal.hs:124-132)."""
        # the 5-tuple carries no lengths: the C side reads pointers[ncols] indices and values, so a last pointer
        # beyond the arrays (or a pointer array shorter than ncols + 1) would be a heap over-read before any
        # validation on the device could refuse the matrix
        if len(self.pointers) != self.ncols + 1:
            _oops("withConstMatrix", "pointers has %d entries for %d columns" % (len(self.pointers), self.ncols))
        nz = int(self.pointers[-1]) if len(self.pointers) else 0
        if nz < 0 or nz > len(self.indices) or nz > len(self.values):
            _oops("withConstMatrix", "last pointer %d, but %d indices and %d values" % (nz, len(self.indices), len(self.values)))
        vals = self.values.view(F64) if self.is_complex else self.values
        # The reference narrows its 64-bit Int arrays on EVERY call (Foreign.hs:39-41: 2.4 GB of conversion per FFI call at
        # config C2).  A Matrix is a value — the fields of the Haskell record cannot change — so the
        # mirror narrows once and keeps the int32 copies while `pointers` and `indices` are the objects they were
        # (round 4: at config C5 the copy was 30 ms of every 170 ms `linearSolve_`).  The fields are read-only views, so
        # an edit through the Matrix raises; an edit through another alias of the caller's buffer is looked for on every
        # call by a fingerprint of the pattern (lengths, last pointer, ~4 000 evenly spaced entries: microseconds) — a
        # mismatch narrows again.  (identity alone let a stale pattern through.)
        kept = getattr(self, "_narrowed", None)
        if (kept is None or kept[0] is not self.pointers or kept[1] is not self.indices
                or not _same_fingerprint(kept[4], _pattern_fingerprint(self.pointers, self.indices))):
            kept = (self.pointers, self.indices, as_i32(self.pointers), as_i32(self.indices),
                    _pattern_fingerprint(self.pointers, self.indices))
            try:
                self._narrowed = kept
            except AttributeError:  # (a subclass with __slots__)
                pass
        return (self.nrows, self.ncols, kept[2], kept[3], as_f64(vals))

    def _parts(self):
        """real and imaginary parts as two real matrices with the same pattern"""
        return (Matrix(self.ncols, self.nrows, self.pointers, self.indices, self.values.real.copy()),
                Matrix(self.ncols, self.nrows, self.pointers, self.indices, self.values.imag.copy()))

    def device_handle(self):
        """Upload once, reuse for every later SpMV (handle API)."""
        if self._handle is None:
            if self.is_complex:
                self._handle = DeviceMatrix.from_csc_complex(self)
            else:
                self._handle = DeviceMatrix.from_csc(self)
                self._handle.optimize()  # one-time analysis, like umfpack_*_symbolic
        return self._handle


class DeviceMatrix(_ffi.Handle):
    """Owner of a ``void *H`` from ``spl_matrix_create*`` (UMFPACK-style handle:
    callee-allocated, freed through ``void **``; Umfpack.hs:63-65)."""
    ORDER_REFERENCE = 0
    ORDER_FREE = 1
    # the `form` argument of build_panel (SPL_PANEL_FORM_* of include/sparse_linear_hip.h)
    PANEL_FORM_DEFAULT = 0
    PANEL_FORM_CHUNK_K1, PANEL_FORM_CHUNK_K2 = 1, 2
    PANEL_FORM_PAIRED_K1, PANEL_FORM_PAIRED_K2 = 4, 5
    PANEL_FORM_RING_K1, PANEL_FORM_RING_K2, PANEL_FORM_RING_K3, PANEL_FORM_RING_K4, PANEL_FORM_RING_K8 = 6, 7, 8, 9, 10
    PANEL_FORM_ROUNDS = 11

    def __init__(self, handle):
        _ffi.Handle.__init__(self, "spl_matrix_free", handle)

    @classmethod
    def from_csc(cls, mat, part=0, nparts=1):
        _ffi.require_gpu()
        nr, nc, ap, ai, ax = mat._tuple32()
        h = C.c_void_p()
        check("spl_matrix_create_rowblock",
              lib().spl_matrix_create_rowblock(nr, nc, p_i32(ap), p_i32(ai), p_f64(ax), part, nparts,
                                               C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_csc_complex(cls, mat):
        """Complex Double handle (spl_matrix_create_z): packed (re, im) values, native SpMV (csrc/spmv_z.hip)"""
        _ffi.require_gpu()
        nr, nc, ap, ai, az = mat._tuple32()  # complex values cross as packed pairs
        h = C.c_void_p()
        check("spl_matrix_create_z", lib().spl_matrix_create_z(nr, nc, p_i32(ap), p_i32(ai), p_f64(az), C.byref(h)))
        return cls(h.value)

    @property
    def is_complex(self):
        return int(lib().spl_matrix_is_complex(self.handle)) == 1

    @classmethod
    def from_csr(cls, nrows_global, ncols, rowptr, colidx, val, row0=0):
        _ffi.require_gpu()
        rp, ci, v = as_i32(rowptr), as_i32(colidx), as_f64(val)
        if len(rp) < 1 or int(rp[-1]) < 0 or int(rp[-1]) > len(ci) or int(rp[-1]) > len(v):
            _oops("from_csr", "last row pointer %s, but %d column indices and %d values" % (rp[-1] if len(rp) else None, len(ci), len(v)))
        h = C.c_void_p()
        check("spl_matrix_create_csr",
              lib().spl_matrix_create_csr(nrows_global, ncols, row0, len(rp) - 1, p_i32(rp), p_i32(ci),
                                          p_f64(v), C.byref(h)))
        return cls(h.value)

    @classmethod
    def synthetic(cls, kind, n_or_m, K=20, seed=0x5EED, row0=0, row1=None):
        """kind: 'random' | 'banded' | 'poisson2d' | 'poisson3d' (include/spl_synth.h)."""
        _ffi.require_gpu()
        kinds = {"random": 0, "banded": 1, "poisson2d": 2, "poisson3d": 3}
        k = kinds[kind]
        n = n_or_m ** 2 if k == 2 else n_or_m ** 3 if k == 3 else n_or_m
        row1 = n if row1 is None else row1
        h = C.c_void_p()
        check("spl_matrix_create_synthetic",
              lib().spl_matrix_create_synthetic(k, n_or_m, K, seed, row0, row1, C.byref(h)))
        return cls(h.value)

    @classmethod
    def rmat(cls, scale, edge_factor=32, abc=(0.25, 0.25, 0.25), seed=0x5EED):
        _ffi.require_gpu()
        h = C.c_void_p()
        check("spl_matrix_create_rmat",
              lib().spl_matrix_create_rmat(scale, edge_factor, abc[0], abc[1], abc[2], seed, C.byref(h)))
        return cls(h.value)

    def spgemm(self, other):
        """device-resident C = self * other, both real or both complex; returns (DeviceMatrix C, number of products)"""
        h = C.c_void_p()
        prod = C.c_int64(0)
        check("spl_matrix_spgemm", lib().spl_matrix_spgemm(self.handle, other.handle, C.byref(h), C.byref(prod)))
        return DeviceMatrix(h.value), int(prod.value)

    def lin(self, alpha, other, beta):
        """device-resident alpha * self + beta * other (Sparse.hs:401-431): handle in, handle out"""
        h = C.c_void_p()
        a = (C.c_double * 2)(complex(alpha).real, complex(alpha).imag)
        b = (C.c_double * 2)(complex(beta).real, complex(beta).imag)
        check("spl_matrix_lin", lib().spl_matrix_lin(self.handle, a, other.handle, b, C.byref(h)))
        return DeviceMatrix(h.value)

    def to_complex(self):
        """the Complex Double handle (x :+ 0) of a real one"""
        h = C.c_void_p()
        check("spl_matrix_to_complex", lib().spl_matrix_to_complex(self.handle, C.byref(h)))
        return DeviceMatrix(h.value)

    def transpose(self):
        """device-resident transpose (Sparse.hs:301-329), real or complex; whole matrices"""
        h = C.c_void_p()
        check("spl_matrix_transpose", lib().spl_matrix_transpose(self.handle, C.byref(h)))
        return DeviceMatrix(h.value)

    def ctrans(self):
        """device-resident conjugate transpose (Sparse.hs:371-375); on a real handle the transpose"""
        h = C.c_void_p()
        check("spl_matrix_ctrans", lib().spl_matrix_ctrans(self.handle, C.byref(h)))
        return DeviceMatrix(h.value)

    def hermitian(self):
        """`ctrans m == m` (Sparse.hs:377-379) decided on the device without building ctrans m; synchronises"""
        r = C.c_int(0)
        check("spl_matrix_hermitian", lib().spl_matrix_hermitian(self.handle, C.byref(r)))
        return bool(r.value)

    def kronecker(self, other):
        """device-resident Kronecker product self (x) other (Sparse.hs:597-634), both real or both complex; whole
        matrices.  nnz may exceed 2^31"""
        h = C.c_void_p()
        check("spl_matrix_kronecker", lib().spl_matrix_kronecker(self.handle, other.handle, C.byref(h)))
        return DeviceMatrix(h.value)

    @classmethod
    def assemble(cls, blocks, row_off, col_off, nrows, ncols):
        """block b placed at (row_off[b], col_off[b]) of an nrows x ncols result (spl_matrix_assemble_blocks): disjoint
        rectangles in any order, all real or all complex; no block at all gives `zeros`"""
        blocks = list(blocks)
        k = len(blocks)
        if k == 0:
            _ffi.require_gpu()
        hs = (C.c_void_p * max(k, 1))(*[b.handle.value for b in blocks])
        ro = np.ascontiguousarray(row_off, dtype=I64).reshape(-1)
        co = np.ascontiguousarray(col_off, dtype=I64).reshape(-1)
        if len(ro) != k or len(co) != k:
            _oops("assemble", "%d blocks, but %d row offsets and %d column offsets" % (k, len(ro), len(co)))
        h = C.c_void_p()
        check("spl_matrix_assemble_blocks",
              lib().spl_matrix_assemble_blocks(k, hs, _ffi.p_i64(ro), _ffi.p_i64(co), int(nrows), int(ncols), C.byref(h)))
        return cls(h.value)

    @classmethod
    def hcat(cls, mats):
        """hcat (Sparse.hs:504-522) of handles"""
        mats = list(mats)
        if not mats:
            _oops("hcat", "empty list")
        dims = [(m.info()["nrows_global"], m.info()["ncols"]) for m in mats]
        if any(d[0] != dims[0][0] for d in dims):
            _oops("hcat", "nrows mismatch")
        widths = [d[1] for d in dims]
        return cls.assemble(mats, [0] * len(mats), np.concatenate([[0], np.cumsum(widths)])[:-1], dims[0][0], sum(widths))

    @classmethod
    def vcat(cls, mats):
        """vcat (Sparse.hs:528-559) of handles"""
        mats = list(mats)
        if not mats:
            _oops("vcat", "empty list")
        dims = [(m.info()["nrows_global"], m.info()["ncols"]) for m in mats]
        if any(d[1] != dims[0][1] for d in dims):
            _oops("vcat", "ncols mismatch")
        heights = [d[0] for d in dims]
        return cls.assemble(mats, np.concatenate([[0], np.cumsum(heights)])[:-1], [0] * len(mats), sum(heights), dims[0][1])

    @classmethod
    def from_blocks(cls, blocks):
        """fromBlocks (Sparse.hs:563-587) on a grid of handles, None = zero block: the dimension rules and messages of
        the host fromBlocks, the dimensions taken from info()"""
        dims = {}

        def dim(m, key):
            if id(m) not in dims:
                dims[id(m)] = m.info()
            return dims[id(m)][key]

        placed, ro, co, nrows, ncols = _block_grid(blocks, lambda m: dim(m, "nrows_global"), lambda m: dim(m, "ncols"))
        return cls.assemble(placed, ro, co, nrows, ncols)

    @classmethod
    def from_blocks_diag(cls, blocks):
        """fromBlocksDiag (Sparse.hs:589-597): a grid of handles given by (super-)diagonals"""
        return cls.from_blocks(_diag_grid(blocks))

    @classmethod
    def block_diag(cls, mats):
        """blockDiag (Sparse.hs:661-667): one placement, however many blocks"""
        mats = list(mats)
        n = len(mats)
        return cls.from_blocks_diag([mats] + [[None] * n for _ in range(n - 1)])

    def submatrix(self, r0, c0, nr, nc):
        """the window self[r0 : r0 + nr, c0 : c0 + nc] as a handle of its own, indices relative to the window
        (spl_matrix_submatrix): what `subMatrix (r0, c0) (nr, nc)` of the reference documents; whole matrices, real or
        complex; nothing crosses PCIe"""
        h = C.c_void_p()
        check("spl_matrix_submatrix",
              lib().spl_matrix_submatrix(self.handle, int(r0), int(c0), int(nr), int(nc), C.byref(h)))
        return DeviceMatrix(h.value)

    def select(self, rows=None, cols=None):
        """C[i, j] = self[rows[i], cols[j]] as a handle (spl_matrix_select).  rows / cols: torch int32 or int64 tensors
        on the handle's device, or anything torch.as_tensor takes (uploaded as int64); None = all of them in order.
        rows may repeat, cols may not; every result row ascends whatever the order of cols.  A permutation P A Q is
        select(p, q)"""
        import torch
        inf = self.info()
        dev = torch.device("cuda", inf["device"])

        def index_tensor(a, what):
            if a is None:
                return None
            if not isinstance(a, torch.Tensor):
                a = torch.as_tensor(a, dtype=torch.int64)
            if a.dtype not in (torch.int32, torch.int64):
                raise TypeError("select: %s of dtype %s; int32 or int64 is needed" % (what, a.dtype))
            if a.dim() != 1:
                raise TypeError("select: %s with %d dimensions; a 1-D index array is needed" % (what, a.dim()))
            return a.to(dev).contiguous()

        with torch.cuda.device(dev):
            ti, tj = index_tensor(rows, "rows"), index_tensor(cols, "cols")
            if ti is not None and tj is not None and ti.dtype != tj.dtype:  # one width for both arrays
                ti, tj = ti.to(torch.int64), tj.to(torch.int64)
            given = ti if ti is not None else tj
            width = 4 if given is not None and given.dtype == torch.int32 else 8
            n_i = inf["nrows_global"] if ti is None else int(ti.shape[0])
            n_j = inf["ncols"] if tj is None else int(tj.shape[0])
            # an empty tensor has no storage to point at; any aligned non-NULL address says "given, and empty"
            p_i = None if ti is None else C.c_void_p(ti.data_ptr() if n_i else 8)
            p_j = None if tj is None else C.c_void_p(tj.data_ptr() if n_j else 8)
            torch.cuda.current_stream().synchronize()  # the call runs on the default stream
            h = C.c_void_p()
            bad = C.c_int64(-1)
            st = lib().spl_matrix_select(self.handle, n_i, p_i, n_j, p_j, width, C.byref(h), C.byref(bad))
        if st == SPL_ERROR_index_out_of_bounds:
            raise _ffi.SparseLinearError("spl_matrix_select", st, "first offending position: %d" % bad.value)
        check("spl_matrix_select", st)
        return DeviceMatrix(h.value)

    def __getitem__(self, key):
        """self[a:b, c:d] (step 1 or None) is submatrix; self[rows, cols] with two 1-D index tensors or lists is select.
        Strided slices, masks, scalars and mixtures are not served: TypeError"""
        import builtins
        if not (isinstance(key, tuple) and len(key) == 2):
            raise TypeError("DeviceMatrix[...] takes a pair: two slices, or two index arrays")
        a, b = key
        if isinstance(a, builtins.slice) and isinstance(b, builtins.slice):
            if a.step not in (None, 1) or b.step not in (None, 1):
                raise TypeError("DeviceMatrix[...]: strided slices are not served")
            inf = self.info()
            r0, r1, _ = a.indices(inf["nrows_global"])
            c0, c1, _ = b.indices(inf["ncols"])
            return self.submatrix(r0, c0, max(r1 - r0, 0), max(c1 - c0, 0))

        def is_index_array(v):
            if isinstance(v, (list, tuple, np.ndarray)):
                v = np.asarray(v)
                return v.ndim == 1 and (v.size == 0 or v.dtype.kind in "iu")
            return hasattr(v, "dim") and hasattr(v, "data_ptr") and v.dim() == 1 and not v.dtype.is_floating_point \
                and str(v.dtype) in ("torch.int32", "torch.int64")

        if is_index_array(a) and is_index_array(b):
            as_ix = lambda v: np.asarray(v, dtype=I64) if isinstance(v, (list, tuple, np.ndarray)) else v  # noqa: E731
            return self.select(as_ix(a), as_ix(b))
        raise TypeError("DeviceMatrix[...] takes two slices with step 1, or two 1-D index arrays")

    # ---- the entry-wise layer (csrc/entrywise.hip): maps, scaling, filters, reductions; row blocks are accepted ----
    MAP_OPS = {"negate": _ffi.SPL_MAP_negate, "abs": _ffi.SPL_MAP_abs, "signum": _ffi.SPL_MAP_signum,
               "conj": _ffi.SPL_MAP_conj, "real": _ffi.SPL_MAP_real, "imag": _ffi.SPL_MAP_imag,
               "scale": _ffi.SPL_MAP_scale}

    def map(self, op, scalar=None):
        """`cmap` with one of the reference's own functions on the device (spl_matrix_map): op is 'negate', 'abs',
        'signum', 'conj', 'real', 'imag' or 'scale' (with `scalar`).  The pattern stays, stored zeros included; on a
        complex handle 'real' and 'imag' give real handles and 'abs' is `magnitude z :+ 0`"""
        if op not in self.MAP_OPS:
            raise ValueError("map: op %r; one of %s is needed" % (op, ", ".join(sorted(self.MAP_OPS))))
        s = None
        if op == "scale":
            if scalar is None:
                raise ValueError("map: 'scale' needs a scalar")
            s = (C.c_double * 2)(complex(scalar).real, complex(scalar).imag)
        h = C.c_void_p()
        check("spl_matrix_map", lib().spl_matrix_map(self.handle, self.MAP_OPS[op], s, C.byref(h)))
        return DeviceMatrix(h.value)

    def negate(self):
        return self.map("negate")

    def abs(self):
        return self.map("abs")

    def signum(self):
        return self.map("signum")

    def conj(self):
        return self.map("conj")

    def real(self):
        return self.map("real")

    def imag(self):
        return self.map("imag")

    def scale(self, x):
        """`scale x` (Sparse.hs:123-125): every stored value times x; a scalar with an imaginary part needs a complex
        handle (to_complex first, the rule of lin)"""
        return self.map("scale", x)

    def __neg__(self):
        return self.map("negate")

    def __abs__(self):
        return self.map("abs")

    def scale_rows_cols(self, r=None, c=None):
        """diag(r) self diag(c) as a handle (spl_matrix_scale_rows_cols): C[i, j] = (r[i] * a[i, j]) * c[j].  r / c:
        torch tensors on the handle's device, or anything torch.as_tensor takes; float64 on a real handle, float64 or
        complex128 on a complex one; nrows_local and ncols entries; None = ones, and that product is not formed"""
        import torch
        inf = self.info()
        dev = torch.device("cuda", inf["device"])
        cplx = self.is_complex
        want = torch.complex128 if cplx else torch.float64

        def vector(a, n, what):
            if a is None:
                return None
            if not isinstance(a, torch.Tensor):
                a = torch.as_tensor(np.asarray(a))  # a list of Python floats is float64, as numpy reads it
            if a.dtype not in ((torch.float64, torch.complex128) if cplx else (torch.float64,)):
                raise TypeError("scale_rows_cols: %s of dtype %s; %s is needed" % (what, a.dtype, want))
            if a.dim() != 1:
                raise TypeError("scale_rows_cols: %s with %d dimensions; a vector is needed" % (what, a.dim()))
            if int(a.shape[0]) != n:
                raise ValueError("scale_rows_cols: %s has %d entries, %d are needed" % (what, int(a.shape[0]), n))
            return a.to(device=dev, dtype=want).contiguous()

        with torch.cuda.device(dev):
            tr, tc = vector(r, inf["nrows_local"], "r"), vector(c, inf["ncols"], "c")
            p_r = None if tr is None or tr.numel() == 0 else C.c_void_p(tr.data_ptr())
            p_c = None if tc is None or tc.numel() == 0 else C.c_void_p(tc.data_ptr())
            torch.cuda.current_stream().synchronize()  # the call runs on the default stream
            h = C.c_void_p()
            check("spl_matrix_scale_rows_cols", lib().spl_matrix_scale_rows_cols(self.handle, p_r, p_c, C.byref(h)))
        return DeviceMatrix(h.value)

    def drop_zeros(self):
        """the handle without its stored zeros (spl_matrix_filter, SPL_KEEP_nonzero): +0.0 and -0.0 go, NaN stays, a
        complex entry goes iff both parts are zero; the order inside the rows is kept"""
        h = C.c_void_p()
        check("spl_matrix_filter", lib().spl_matrix_filter(self.handle, _ffi.SPL_KEEP_nonzero, None, C.byref(h)))
        return DeviceMatrix(h.value)

    def drop_small(self, tol):
        """the handle without the entries with |a| <= tol (SPL_KEEP_abs_above); NaN entries stay"""
        t = (C.c_double * 1)(float(tol))
        h = C.c_void_p()
        check("spl_matrix_filter", lib().spl_matrix_filter(self.handle, _ffi.SPL_KEEP_abs_above, t, C.byref(h)))
        return DeviceMatrix(h.value)

    def band(self, lo=None, hi=None):
        """the entries with lo <= j - i <= hi, i the global row (spl_matrix_band); None opens an end; lo > hi gives
        `zeros` of the shape"""
        i64 = np.iinfo(np.int64)
        lo = i64.min if lo is None else min(max(int(lo), i64.min), i64.max)
        hi = i64.max if hi is None else min(max(int(hi), i64.min), i64.max)
        h = C.c_void_p()
        check("spl_matrix_band", lib().spl_matrix_band(self.handle, lo, hi, C.byref(h)))
        return DeviceMatrix(h.value)

    def tril(self, k=0):
        """the entries on and below the k-th diagonal: j - i <= k"""
        return self.band(None, k)

    def triu(self, k=0):
        """the entries on and above the k-th diagonal: j - i >= k"""
        return self.band(k, None)

    def _reduce(self, what, axis):
        import torch
        if axis not in (0, 1):
            raise ValueError("axis %r; 0 (per column) or 1 (per row) is needed" % (axis,))
        inf = self.info()
        n = inf["nrows_local"] if axis == 1 else inf["ncols"]
        with torch.cuda.device(inf["device"]):
            out = torch.empty(n, dtype=torch.float64, device="cuda")
            check("spl_matrix_reduce_dev",
                  lib().spl_matrix_reduce_dev(self.handle, what, axis, C.c_void_p(out.data_ptr() if n else 0),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def abs_sums(self, axis):
        """sum of |a| over every row (axis 1) or column (axis 0) as a float64 torch tensor on the device, in a fixed
        order: two calls give the same bits.  Enqueued on torch's current stream"""
        return self._reduce(_ffi.SPL_REDUCE_abs_sum, axis)

    def abs_max(self, axis):
        """largest |a| of every row (axis 1) or column (axis 0), exact; an empty slice gives 0, a NaN is carried"""
        return self._reduce(_ffi.SPL_REDUCE_abs_max, axis)

    def norm(self, which="fro"):
        """1 (largest column abs-sum), inf (largest row abs-sum), 'fro' or 'max', as a float; whole matrices"""
        codes = {1: _ffi.SPL_NORM_one, "1": _ffi.SPL_NORM_one, float("inf"): _ffi.SPL_NORM_inf,
                 "inf": _ffi.SPL_NORM_inf, "fro": _ffi.SPL_NORM_fro, "max": _ffi.SPL_NORM_max}
        if which not in codes:
            raise ValueError("norm: %r; one of 1, inf, 'fro', 'max' is needed" % (which,))
        r = C.c_double(0.0)
        check("spl_matrix_norm", lib().spl_matrix_norm(self.handle, codes[which], C.byref(r)))
        return float(r.value)

    def take_diag_dev(self, out_ptr, stream=0):
        """out[c] = A[c, c] or 0, c < min(nrows, ncols) (Sparse.hs:640-650); out_ptr is a device pointer (int) to
        doubles, or packed (re, im) pairs on a complex handle; enqueues on `stream`, no sync"""
        check("spl_matrix_take_diag_dev",
              lib().spl_matrix_take_diag_dev(self.handle, C.c_void_p(out_ptr), C.c_void_p(stream)))

    def take_diag(self):
        """the diagonal as a numpy vector (float64 or complex128)"""
        import torch
        inf = self.info()
        n = min(inf["nrows_global"], inf["ncols"])
        cplx = self.is_complex
        with torch.cuda.device(inf["device"]):
            out = torch.empty(max(n, 1), dtype=torch.complex128 if cplx else torch.float64, device="cuda")
            self.take_diag_dev(out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            return out[:n].cpu().numpy()

    @classmethod
    def diag_dev(cls, n, values_ptr=None, complex=False):
        """diag (Sparse.hs:652-659) of n values in device memory (doubles, or packed pairs with complex=True);
        values_ptr None: ones"""
        h = C.c_void_p()
        check("spl_matrix_diag_dev",
              lib().spl_matrix_diag_dev(int(n), C.c_void_p(values_ptr), 2 if complex else 1, C.byref(h)))
        return cls(h.value)

    @classmethod
    def ident(cls, n, complex=False):
        """ident n (Sparse.hs:669-671), made on the device"""
        return cls.diag_dev(n, None, complex)

    @classmethod
    def compress_dev(cls, nrows, ncols, ntriples, rows_ptr, cols_ptr, vals_ptr, index_width=4, complex=False):
        """COO triples in device memory -> handle (Sparse.hs:184-280).  The default is int32 indices and float64 values
        (spl_matrix_compress_dev); index_width=8 takes int64 indices, complex=True packed (re, im) pairs
        (spl_matrix_compress_dev_wide)"""
        _ffi.require_gpu()
        h = C.c_void_p()
        bad = C.c_int64(-1)
        if index_width == 4 and not complex:
            st = lib().spl_matrix_compress_dev(nrows, ncols, ntriples, C.c_void_p(rows_ptr), C.c_void_p(cols_ptr),
                                               C.c_void_p(vals_ptr), C.byref(h), C.byref(bad))
            check("spl_matrix_compress_dev", st)
        else:
            st = lib().spl_matrix_compress_dev_wide(nrows, ncols, ntriples, int(index_width), C.c_void_p(rows_ptr),
                                                    C.c_void_p(cols_ptr), C.c_void_p(vals_ptr), 2 if complex else 1,
                                                    C.byref(h), C.byref(bad))
            if st == SPL_ERROR_index_out_of_bounds:
                raise _ffi.SparseLinearError("spl_matrix_compress_dev_wide", st, "first offending triple: %d" % bad.value)
            check("spl_matrix_compress_dev_wide", st)
        return cls(h.value)

    @classmethod
    def from_csr_dev(cls, nrows, ncols, rowptr_ptr, colidx_ptr, val_ptr, index_width=4, complex=False):
        """CSR arrays in device memory (device pointers as ints; int32 or int64 pointers and indices, float64 values or
        packed pairs) -> whole-matrix handle (spl_matrix_create_csr_dev).  The arrays are copied; synchronises"""
        _ffi.require_gpu()
        h = C.c_void_p()
        check("spl_matrix_create_csr_dev",
              lib().spl_matrix_create_csr_dev(int(nrows), int(ncols), int(index_width), C.c_void_p(rowptr_ptr),
                                              C.c_void_p(colidx_ptr), C.c_void_p(val_ptr), 2 if complex else 1,
                                              C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_csc_dev(cls, nrows, ncols, colptr_ptr, rowidx_ptr, val_ptr, index_width=4, complex=False):
        """the reference's CSC fields in device memory -> whole-matrix handle (spl_matrix_create_csc_dev)"""
        _ffi.require_gpu()
        h = C.c_void_p()
        check("spl_matrix_create_csc_dev",
              lib().spl_matrix_create_csc_dev(int(nrows), int(ncols), int(index_width), C.c_void_p(colptr_ptr),
                                              C.c_void_p(rowidx_ptr), C.c_void_p(val_ptr), 2 if complex else 1,
                                              C.byref(h)))
        return cls(h.value)

    def export_csr_dev(self, rowptr_ptr, colidx_ptr, val_ptr, index_width=4):
        """the arrays of export_csr written into device memory the caller allocated: rowptr[nrows_local + 1] and
        colidx[nnz] of index_width bytes per element, val[nnz] doubles (2 nnz on a complex handle); synchronises"""
        check("spl_matrix_export_csr_dev",
              lib().spl_matrix_export_csr_dev(self.handle, int(index_width), C.c_void_p(rowptr_ptr),
                                              C.c_void_p(colidx_ptr), C.c_void_p(val_ptr)))

    def export_csc_dev(self, colptr_ptr, rowidx_ptr, val_ptr, index_width=4):
        """the reference's CSC fields written into device memory: colptr[ncols + 1], rowidx[nnz], val[nnz] (2 nnz doubles
        on a complex handle, which export_csc does not serve); synchronises"""
        check("spl_matrix_export_csc_dev",
              lib().spl_matrix_export_csc_dev(self.handle, int(index_width), C.c_void_p(colptr_ptr),
                                              C.c_void_p(rowidx_ptr), C.c_void_p(val_ptr)))

    @classmethod
    def from_torch(cls, t):
        """handle of a 2-D torch.sparse_csr / sparse_csc / sparse_coo tensor on a GPU, float64 or complex128, int32 or
        int64 indices, without a host copy.  COO triples go through compress as they are (no coalesce(): duplicates are
        summed in input order).  Nothing is cast or moved silently: other dtypes, CPU tensors, batch or dense dimensions
        and strided tensors are refused.  Synchronises torch's current stream, then the import runs on the tensor's
        device"""
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError("from_torch: a torch.Tensor is needed, got %s" % type(t).__name__)
        layouts = (torch.sparse_csr, torch.sparse_csc, torch.sparse_coo)
        if t.layout not in layouts:
            raise TypeError("from_torch: layout %s; sparse_csr, sparse_csc or sparse_coo is needed" % t.layout)
        if t.dtype not in (torch.float64, torch.complex128):
            raise TypeError("from_torch: dtype %s; float64 or complex128 is needed (nothing is cast)" % t.dtype)
        if t.dim() != 2:
            raise ValueError("from_torch: %d dimensions; batch dimensions are not served" % t.dim())
        if t.dense_dim() != 0:
            raise ValueError("from_torch: dense (hybrid) dimensions are not served")
        if t.device.type != "cuda":
            raise ValueError("from_torch: the tensor is on %s; it is not moved to a GPU silently" % t.device)
        nrows, ncols = int(t.shape[0]), int(t.shape[1])
        cplx = t.dtype == torch.complex128
        if t.layout == torch.sparse_csr:
            ptr, idx, val = t.crow_indices(), t.col_indices(), t.values()
        elif t.layout == torch.sparse_csc:
            ptr, idx, val = t.ccol_indices(), t.row_indices(), t.values()
        else:
            ptr, idx, val = None, t._indices(), t._values()
        if idx.dtype not in (torch.int32, torch.int64):
            raise TypeError("from_torch: index dtype %s" % idx.dtype)
        width = 8 if idx.dtype == torch.int64 else 4
        with torch.cuda.device(t.device):
            idx, val = idx.contiguous(), val.contiguous()  # copies on the device, and only when needed
            if ptr is None:
                rows, cols = idx[0], idx[1]  # contiguous rows of the 2 x nnz index tensor
                n = int(val.shape[0])
                torch.cuda.current_stream().synchronize()
                return cls.compress_dev(nrows, ncols, n, rows.data_ptr() if n else 0, cols.data_ptr() if n else 0,
                                        val.data_ptr() if n else 0, index_width=width, complex=cplx)
            ptr = ptr.contiguous()
            torch.cuda.current_stream().synchronize()
            make = cls.from_csr_dev if t.layout == torch.sparse_csr else cls.from_csc_dev
            return make(nrows, ncols, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), index_width=width, complex=cplx)

    def to_torch(self, layout=None, index_dtype=None):
        """the matrix as a torch.sparse_csr (default) or sparse_csc tensor on the handle's device, index_dtype
        torch.int64 (default) or torch.int32, values float64 or, for a complex handle, complex128 over the packed pairs.
        The three tensors are allocated by torch and filled on the device.  Whole matrices only"""
        import torch
        layout = torch.sparse_csr if layout is None else layout
        index_dtype = torch.int64 if index_dtype is None else index_dtype
        if layout not in (torch.sparse_csr, torch.sparse_csc):
            raise ValueError("to_torch: layout %s; torch.sparse_csr or torch.sparse_csc is needed" % layout)
        if index_dtype not in (torch.int32, torch.int64):
            raise TypeError("to_torch: index dtype %s; torch.int32 or torch.int64 is needed" % index_dtype)
        inf = self.info()
        if inf["row0"] != 0 or inf["nrows_local"] != inf["nrows_global"]:
            raise ValueError("to_torch: a row block (rows %d .. %d of %d) is not a whole matrix"
                             % (inf["row0"], inf["row0"] + inf["nrows_local"], inf["nrows_global"]))
        nrows, ncols, nnz = inf["nrows_global"], inf["ncols"], inf["nnz"]
        csr = layout == torch.sparse_csr
        dev = torch.device("cuda", inf["device"])
        with torch.cuda.device(dev):
            ptr = torch.empty((nrows if csr else ncols) + 1, dtype=index_dtype, device=dev)
            idx = torch.empty(nnz, dtype=index_dtype, device=dev)
            val = torch.empty(nnz, dtype=torch.complex128 if self.is_complex else torch.float64, device=dev)
            torch.cuda.current_stream().synchronize()
            export = self.export_csr_dev if csr else self.export_csc_dev
            export(ptr.data_ptr(), idx.data_ptr() if nnz else 0, val.data_ptr() if nnz else 0,
                   index_width=8 if index_dtype == torch.int64 else 4)
            make = torch.sparse_csr_tensor if csr else torch.sparse_csc_tensor
            return make(ptr, idx, val, size=(nrows, ncols))

    def info(self):
        buf = (C.c_int64 * 8)()
        check("spl_matrix_info", lib().spl_matrix_info(self.handle, buf))
        keys = ("nrows_global", "ncols", "row0", "nrows_local", "nnz", "device", "blocked_rows", "blocked_cols_log2")
        return dict(zip(keys, [int(v) for v in buf]))

    def export_csr(self):
        inf = self.info()
        rp = np.zeros(inf["nrows_local"] + 1, dtype=I64)
        ci = np.zeros(max(inf["nnz"], 1), dtype=np.int32)
        vw = 2 if self.is_complex else 1
        v = np.zeros(max(inf["nnz"], 1) * vw, dtype=F64)
        check("spl_matrix_export_csr", lib().spl_matrix_export_csr(self.handle, _ffi.p_i64(rp), p_i32(ci), p_f64(v)))
        if vw == 2:
            return rp, ci[:inf["nnz"]], v[:2 * inf["nnz"]].view(np.complex128)
        return rp, ci[:inf["nnz"]], v[:inf["nnz"]]

    def export_csr_rows(self, row0, row1):
        """rows [row0, row1) of the device CSR image: (rowptr relative to the window, colidx, val)"""
        rp = np.zeros(row1 - row0 + 1, dtype=I64)
        st = lib().spl_matrix_export_csr_rows(self.handle, row0, row1, _ffi.p_i64(rp), 0, None, None)
        cnt = int(rp[-1] - rp[0])
        if cnt == 0:
            check("spl_matrix_export_csr_rows", st)
            return rp - rp[0], np.zeros(0, dtype=np.int32), np.zeros(0, dtype=F64)
        ci = np.zeros(cnt, dtype=np.int32)
        v = np.zeros(cnt, dtype=F64)
        check("spl_matrix_export_csr_rows",
              lib().spl_matrix_export_csr_rows(self.handle, row0, row1, _ffi.p_i64(rp), cnt, p_i32(ci), p_f64(v)))
        return rp - rp[0], ci, v

    def export_csc(self):
        """the block as the reference's CSC fields (device transpose, Sparse.hs:301-329)"""
        inf = self.info()
        cp = np.zeros(inf["ncols"] + 1, dtype=I64)
        ri = np.zeros(max(inf["nnz"], 1), dtype=np.int32)
        v = np.zeros(max(inf["nnz"], 1), dtype=F64)
        check("spl_matrix_export_csc", lib().spl_matrix_export_csc(self.handle, _ffi.p_i64(cp), p_i32(ri), p_f64(v)))
        return cp, ri[:inf["nnz"]], v[:inf["nnz"]]

    def set_variant(self, variant):
        check("spl_matrix_set_variant", lib().spl_matrix_set_variant(self.handle, int(variant)))

    def spmm_dev(self, b_ptr, c_ptr, k, accumulate=False, stream=0):
        """C = A B for row-major device arrays B (ncols x k), C (nrows_local x k); no sync"""
        check("spl_matrix_spmm_dev",
              lib().spl_matrix_spmm_dev(self.handle, C.c_void_p(b_ptr), C.c_void_p(c_ptr), int(k),
                                        1 if accumulate else 0, C.c_void_p(stream)))

    def spmv_many_dev(self, x_ptr, ldx, y_ptr, ldy, k, accumulate=False, stream=0):
        """Y[:, j] = A X[:, j] (+ Y[:, j]) for k vectors stored one after the other (column-major device arrays with
        leading dimensions ldx, ldy in entries: doubles, or packed complex pairs on a complex handle); A is read once
        per 16 vectors, every sum in the reference's order (csrc/spmv_many.hip); no sync"""
        check("spl_matrix_spmv_many_dev",
              lib().spl_matrix_spmv_many_dev(self.handle, int(k), C.c_void_p(x_ptr), int(ldx), C.c_void_p(y_ptr),
                                             int(ldy), 1 if accumulate else 0, C.c_void_p(stream)))

    def triangular(self, uplo="lower", unit=False):
        """a TriangularSolver for the lower (j <= i) or upper (j >= i) triangle of this whole square handle
        (spl_trisolve_analyze); the other side of the diagonal is not read, so a Gauss-Seidel sweep passes the full
        matrix.  unit: d_i = 1 and a stored diagonal is ignored.  The handle may be freed afterwards"""
        if uplo not in TriangularSolver.UPLO:
            raise ValueError("triangular: uplo %r; 'lower' or 'upper' is needed" % (uplo,))
        t = C.c_void_p()
        st = check("spl_trisolve_analyze",
                   lib().spl_trisolve_analyze(self.handle, TriangularSolver.UPLO[uplo],
                                              _ffi.SPL_DIAG_unit if unit else _ffi.SPL_DIAG_stored, C.byref(t)))
        return TriangularSolver(t.value, st)

    def ilu0(self):
        """the ILU(0) factorisation of this whole square handle (spl_ilu0_analyze + spl_ilu0_factor): an ILU0 object
        with the factors as a handle of this pattern and the two triangular solvers built from it"""
        return ILU0(self)

    def krylov(self, method="cg", M=None):
        """a KrylovSolver for this whole square handle (spl_krylov_create): 'cg' or 'bicgstab', with the preconditioner
        M (None, an ILU0, 'jacobi', 'sgs' or a (T1, mid, T2) triple).  The handle is borrowed: the solver keeps it alive"""
        return KrylovSolver(self, method, M)

    def gmres(self, restart=30, M=None):
        """a GMRESSolver for this whole square handle (spl_gmres_create): restarted GMRES(restart), 1 ... 128, for
        unsymmetric and indefinite systems, with the preconditioner M as KrylovSolver takes it"""
        return GMRESSolver(self, restart, M)

    def eigsh(self, nev, which="LA", ncv=None, sigma=None, M=None, tol=1e-10, atol=0.0, max_restarts=1000, v0=None,
              inner_rtol=1e-12, inner_atol=0.0, inner_maxiter=None):
        """(values, vectors, result dict): nev eigenpairs of this whole square Hermitian handle by thick-restart Lanczos
        (spl_eigsh_*).  which: 'LA', 'SA' or 'LM' of the operator's values; sigma: work on (A - sigma I)^-1 by CG with the
        preconditioner M, so that 'LM' finds the eigenvalues nearest sigma; ncv: the basis, default
        min(n, max(2 nev + 1, 20)) capped at 128; v0: the start, default numpy.random.default_rng(0).standard_normal"""
        n = self.info()["nrows_global"]
        E = EigenSolver(self, default_ncv(n, nev) if ncv is None else ncv, sigma, M, inner_rtol, inner_atol,
                        inner_maxiter)
        try:
            return E.solve(nev, which, tol, atol, max_restarts, v0)
        finally:
            E.free()

    def lobpcg(self, X0, nev=None, largest=False, M=None, tol=1e-8, atol=0.0, maxiter=200, B=None):
        """(values, vectors, result dict): the nev smallest (largest=True: largest) eigenpairs of this whole square
        Hermitian handle by LOBPCG (spl_lobpcg_*) from the start block X0 (n x block, 1 <= block <= 42; nev defaults to
        the block), with the preconditioner M (as KrylovSolver takes it) applied inside the iteration.  A block method:
        multiple eigenvalues come with their copies.  B: a Hermitian positive definite DeviceMatrix, for
        A x = lambda B x with B-orthonormal vectors"""
        block = int(X0.shape[1]) if getattr(X0, "ndim", 0) == 2 else 0
        L = LOBPCGSolver(self, block, M, B)
        try:
            return L.solve(X0, nev, largest, tol, atol, maxiter)
        finally:
            L.free()

    def coloring(self, seed=0):
        """the multicolour ordering of this whole square handle (spl_matrix_color): a Coloring with colors, perm and
        offsets; ``coloring().krylov(method, M)`` solves with the preconditioner built in that ordering"""
        return Coloring(self, seed)

    @classmethod
    def _borrowed(cls, handle, owner):
        """a view of a handle that `owner` frees: free() and the collector leave the handle alone"""
        view = cls.__new__(cls)
        view._h = C.c_void_p(handle)
        view._finalizer = lambda: None
        view._owner = owner
        return view

    def aggregate(self, seed=0):
        """the aggregation of this whole square handle's graph (spl_matrix_aggregate): a dict with ``agg`` (n) and
        ``roots`` (one per aggregate) as torch int32 device tensors and ``info`` (AMG.AGGREGATE_KEYS)"""
        handle = self.handle
        _ffi.require_gpu()
        import torch
        inf = self.info()
        n = inf["nrows_global"]
        dev = torch.device("cuda", inf["device"])
        out = np.zeros(8, dtype=I64)
        with torch.cuda.device(dev):
            agg = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            roots = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            torch.cuda.current_stream().synchronize()  # the call runs on the default stream
            check("spl_matrix_aggregate",
                  lib().spl_matrix_aggregate(handle, int(seed), C.c_void_p(agg.data_ptr()), C.c_void_p(roots.data_ptr()),
                                             _ffi.p_i64(out)))
        return {"agg": agg[:n], "roots": roots[:int(out[1])], "info": dict(zip(AMG.AGGREGATE_KEYS, (int(v) for v in out)))}

    def amg(self, **options):
        """the aggregation AMG hierarchy of this whole square handle (spl_amg_create): an AMG object; options: seed,
        sweeps, coarse_size, max_levels, coarse_sweeps, plain.  The handle is borrowed: the object keeps it alive"""
        return AMG(self, **options)

    def optimize(self):
        """one-time analysis; may build the column-blocked image (csrc/spmv_blocked.hip)"""
        check("spl_matrix_optimize", lib().spl_matrix_optimize(self.handle))

    def build_blocked(self, rows_per_panel=0, cols_log2=0, unroll=0):
        check("spl_matrix_build_blocked",
              lib().spl_matrix_build_blocked(self.handle, rows_per_panel, cols_log2, unroll))

    def build_panel(self, rows_per_panel=0, cols_log2=0, unroll=0, form=0):
        """the column-sorted panel image (csrc/spmv_panel.hip): order-free sums, 1e-10 contract;
        form (PANEL_FORM_*) CHUNK_K1 / _K2: one chunk per load, 1 / 2 index blocks per phase; PAIRED_K1 / _K2: paired
        storage, 1 / 2 index blocks per phase (the default's heuristic); RING_K1 ... _K8: ring form; ROUNDS: rounds form on
        the paired storage — rounds of exactly 16 * unroll pairs of chunks whatever the index blocks are (unroll 3 ... 6,
        0: 5), no column slices.  What unroll counts per form: include/sparse_linear_hip.h.
        With everything 0 on a large matrix the build times the heuristic's neighbours, the rounds form with and without its rendezvous among them,
        and keeps another candidate only if it is more than 1 % faster."""
        check("spl_matrix_build_panel",
              lib().spl_matrix_build_panel(self.handle, rows_per_panel, cols_log2, unroll, form))

    def panel_errors(self):
        """1 when a bounded wait of the ring form gave up during the last panel SpMV (diagnostics)"""
        r = lib().spl_matrix_panel_errors(self.handle)
        if r < 0:
            check("spl_matrix_panel_errors", r)
        return r

    def set_spmv_order(self, order):
        """ORDER_REFERENCE (0, default): sums in the reference's order, bit-identical; ORDER_FREE (1):
        any order, rounding-level differences (include/sparse_linear_hip.h)"""
        check("spl_matrix_set_spmv_order", lib().spl_matrix_set_spmv_order(self.handle, int(order)))

    def set_reserved_cus(self, reserved):
        """CUs left free for a kernel beside the SpMV (call before optimize(); include/sparse_linear_hip.h)"""
        check("spl_matrix_set_reserved_cus", lib().spl_matrix_set_reserved_cus(self.handle, int(reserved)))

    def spmv_kernel(self):
        """0 CSR-stream, 8 column-blocked lockstep, 15 sliced ELL, 16 column-sorted panels"""
        return int(lib().spl_matrix_spmv_kernel(self.handle))

    def mulv(self, x):
        if self.is_complex:  # packed complex vectors; the lengths count entries
            x = np.ascontiguousarray(x, dtype=C128)
            y = np.zeros(self.info()["nrows_local"], dtype=C128)
            st = lib().spl_matrix_mulv(self.handle, len(x), p_f64(x.view(F64)), p_f64(y.view(F64)))
            if st == SPL_ERROR_dimension_mismatch:
                _oops("axpy_", "column dimension does not match operand dimension %d" % len(x))
            check("spl_matrix_mulv", st)
            return y
        x = as_f64(x)
        y = np.zeros(self.info()["nrows_local"], dtype=F64)
        st = lib().spl_matrix_mulv(self.handle, len(x), p_f64(x), p_f64(y))
        if st == SPL_ERROR_dimension_mismatch:
            _oops("axpy_", "column dimension does not match operand dimension %d" % len(x))
        check("spl_matrix_mulv", st)
        return y

    def gaxpy(self, x, y):
        if self.is_complex:
            x = np.ascontiguousarray(x, dtype=C128)
            assert y.dtype == C128 and y.flags.c_contiguous
            st = lib().spl_matrix_gaxpy(self.handle, len(x), p_f64(x.view(F64)), len(y), p_f64(y.view(F64)))
            if st == SPL_ERROR_dimension_mismatch:
                _oops("axpy_", "dimension does not match operand dimension")
            check("spl_matrix_gaxpy", st)
            return y
        x = as_f64(x)
        assert y.dtype == F64 and y.flags.c_contiguous
        st = lib().spl_matrix_gaxpy(self.handle, len(x), p_f64(x), len(y), p_f64(y))
        if st == SPL_ERROR_dimension_mismatch:
            _oops("axpy_", "dimension does not match operand dimension")
        check("spl_matrix_gaxpy", st)
        return y

    def spmv_dev(self, x_ptr, y_ptr, accumulate=False, stream=0):
        """device pointers (ints); enqueues on `stream` (a hipStream_t as int), no sync"""
        check("spl_matrix_spmv_dev",
              lib().spl_matrix_spmv_dev(self.handle, C.c_void_p(x_ptr), C.c_void_p(y_ptr),
                                        1 if accumulate else 0, C.c_void_p(stream)))


class TriangularSolver(_ffi.Handle):
    """Owner of a ``void *T`` from ``spl_trisolve_analyze``: the level-scheduled solves T x = b, T^T x = b, T^H x = b
    on the device (csrc/trisolve.hip).  Every result is the serial substitution loop bit for bit, whatever the schedule
    and the number of right-hand sides.  ``singular``: the analysis found a missing or zero d_i (the solves then give
    IEEE's inf / NaN, they never refuse)."""
    UPLO = {"lower": _ffi.SPL_TRI_lower, "upper": _ffi.SPL_TRI_upper}
    TRANS = {"N": _ffi.SPL_OP_n, "T": _ffi.SPL_OP_t, "H": _ffi.SPL_OP_h}

    def __init__(self, handle, status=0):
        _ffi.Handle.__init__(self, "spl_trisolve_free", handle)
        self.singular = status == _ffi.SPL_WARNING_singular_matrix

    @classmethod
    def _op(cls, trans):
        if trans not in cls.TRANS:
            raise ValueError("trans %r; 'N', 'T' or 'H' is needed" % (trans,))
        return cls.TRANS[trans]

    def info(self):
        out = np.zeros(8, dtype=I64)
        check("spl_trisolve_info", lib().spl_trisolve_info(self.handle, _ffi.p_i64(out)))
        keys = ("n", "stored", "levels", "launches", "zero_diagonals", "longest_row", "device_bytes", "flags")
        d = dict(zip(keys, (int(v) for v in out)))
        d.update(complex=bool(d["flags"] & 1), upper=bool(d["flags"] & 2), unit=bool(d["flags"] & 4),
                 transposed_built=bool(d["flags"] & 8))
        return d

    def solve_dev(self, b_ptr, ldb, x_ptr, ldx, k, trans="N", stream=0):
        """device pointers (ints) to column-major arrays with leading dimensions in entries (doubles, or packed complex
        pairs); x_ptr == b_ptr with ldx == ldb solves in place; enqueues on `stream`, no sync (the first 'T' / 'H'
        solve builds the transposed image and synchronises)"""
        op = self._op(trans)
        check("spl_trisolve_solve_dev",
              lib().spl_trisolve_solve_dev(self.handle, op, int(k), C.c_void_p(b_ptr), int(ldb), C.c_void_p(x_ptr),
                                           int(ldx), C.c_void_p(stream)))

    def solve(self, b, trans="N"):
        """x with T x = b (trans 'N'), T^T x = b ('T') or T^H x = b ('H').  b: a numpy array (the result is one) or a
        torch tensor on the device (the result is one, enqueued on torch's current stream); 1-D, or 2-D in Fortran order
        (one right-hand side after the other); float64 on a real object, complex128 on a complex one"""
        op = self._op(trans)
        inf = self.info()
        n, cplx = inf["n"], inf["complex"]
        try:
            import torch
            is_tensor = isinstance(b, torch.Tensor)
        except ImportError:  # pragma: no cover
            is_tensor = False
        if is_tensor:
            want = torch.complex128 if cplx else torch.float64
            if b.dtype != want:
                _oops("solveTriangular", "right-hand side of dtype %s; %s is needed" % (b.dtype, want))
            if b.dim() not in (1, 2) or int(b.shape[0]) != n:
                _oops("solveTriangular", "right-hand side of shape %s; %d rows are needed" % (tuple(b.shape), n))
            if not b.is_cuda:
                _oops("solveTriangular", "a torch right-hand side must lie on the device; pass a numpy array otherwise")
            k = 1 if b.dim() == 1 else int(b.shape[1])
            # a column's entries must follow each other whatever k is: an (n, 1) slice of a row-major tensor has
            # strides (k, 1) and is refused like any other row-major operand
            if b.dim() == 2 and n > 1 and (b.stride(0) != 1 or (k > 1 and b.stride(1) < n)):
                _oops("solveTriangular", "a 2-D right-hand side must be in Fortran order (column after column)")
            if b.dim() == 1 and n > 1 and b.stride(0) != 1:
                _oops("solveTriangular", "a 1-D right-hand side must be contiguous")
            with torch.cuda.device(b.device):
                x = torch.empty_strided(tuple(b.shape), (1,) if b.dim() == 1 else (1, max(n, 1)), dtype=want,
                                        device=b.device)
                if n and k:
                    ldb = n if b.dim() == 1 or k == 1 else int(b.stride(1))
                    self.solve_dev(b.data_ptr(), ldb, x.data_ptr(), max(n, 1), k, trans,
                                   torch.cuda.current_stream().cuda_stream)
            return x
        a = np.asarray(b)
        want = C128 if cplx else F64
        if a.dtype != want:
            _oops("solveTriangular", "right-hand side of dtype %s; %s is needed" % (a.dtype, np.dtype(want)))
        if a.ndim not in (1, 2) or a.shape[0] != n:
            _oops("solveTriangular", "right-hand side of shape %s; %d rows are needed" % (a.shape, n))
        if a.ndim == 2 and a.shape[1] > 1 and n > 1 and not a.flags.f_contiguous:
            _oops("solveTriangular", "a 2-D right-hand side must be in Fortran order (column after column)")
        k = 1 if a.ndim == 1 else a.shape[1]
        src = np.ascontiguousarray(a.ravel(order="F"))  # one column after the other; no copy when a is laid out so
        x = np.empty(a.size, dtype=want)
        if n and k:
            check("spl_trisolve_solve",
                  lib().spl_trisolve_solve(self.handle, op, k, p_f64(src.view(F64)), p_f64(x.view(F64))))
        return x.reshape(a.shape, order="F")


def solveTriangular(mat, b, lower=True, unit=False, trans="N"):
    """x with T x = b for the lower / upper triangle T of the host Matrix `mat` (its transpose or conjugate transpose
    with trans 'T' / 'H'), solved on the device; b as TriangularSolver.solve takes it"""
    TriangularSolver._op(trans)
    T = mat.device_handle().triangular("lower" if lower else "upper", unit)
    try:
        return T.solve(b, trans)
    finally:
        T.free()


class ILU0(_ffi.Handle):
    """The incomplete LU factorisation without fill of a whole square device handle (csrc/ilu0.hip): the serial IKJ
    loop bit for bit, whatever the schedule.  ``factors`` is a DeviceMatrix with A's pattern that holds L (unit lower,
    its ones not stored) and U; ``lower`` / ``upper`` are the TriangularSolvers built from it (unit / stored diagonal);
    ``singular``: some final u_kk is missing or exactly zero (the factors then hold IEEE's inf / NaN).  The plan of
    ``spl_ilu0_analyze`` is kept: ``refactor(A)`` factors new values on the same pattern without an analysis."""
    INFO_KEYS = ("n", "nnz", "levels", "launches", "missing_diagonals", "longest_row", "device_bytes", "factorisations")

    def __init__(self, A):
        _ffi.Handle.__init__(self, "spl_ilu0_free")
        self.factors = self.lower = self.upper = None
        self.singular = False
        check("spl_ilu0_analyze", lib().spl_ilu0_analyze(A.handle, C.byref(self._h)))
        self.refactor(A)

    plan = _ffi.Handle.handle  # the handle is the plan of spl_ilu0_analyze

    def _drop_factors(self):
        for part in (self.lower, self.upper, self.factors):
            if part is not None:
                part.free()
        self.factors = self.lower = self.upper = None

    def free(self):
        self._drop_factors()
        _ffi.Handle.free(self)

    def info(self):
        out = np.zeros(8, dtype=I64)
        check("spl_ilu0_info", lib().spl_ilu0_info(self.plan, _ffi.p_i64(out)))
        return dict(zip(self.INFO_KEYS, (int(v) for v in out)))

    def refactor(self, A):
        """new values on the analysed pattern (A: any whole handle with it, real or complex): the factors and the two
        solvers are replaced once all three exist; when a step raises (a handle of another pattern is refused, an
        analysis fails) the object keeps what it had"""
        f = C.c_void_p()
        st = check("spl_ilu0_factor", lib().spl_ilu0_factor(self.plan, A.handle, C.byref(f)))
        factors = DeviceMatrix(f.value)
        lower = upper = None
        try:
            lower = factors.triangular("lower", unit=True)
            upper = factors.triangular("upper")
        except Exception:
            for part in (lower, factors):
                if part is not None:
                    part.free()
            raise
        self._drop_factors()
        self.factors, self.lower, self.upper = factors, lower, upper
        self.singular = st == _ffi.SPL_WARNING_singular_matrix
        return self

    def _solvers(self, trans):
        TriangularSolver._op(trans)
        if self.lower is None or self.upper is None:
            raise _ffi.SparseLinearError("ILU0", _ffi.SPL_ERROR_invalid_handle)
        # (L U)^-1 = U^-1 L^-1;  (L U)^-T = L^-T U^-T
        return (self.lower, self.upper) if trans == "N" else (self.upper, self.lower)

    def apply_dev(self, b_ptr, ldb, x_ptr, ldx, k, trans="N", stream=0):
        """x = U^-1 L^-1 b (trans 'N'), L^-T U^-T b ('T') or L^-H U^-H b ('H') in two solve_dev calls on `stream`, no
        sync; device pointers and leading dimensions as TriangularSolver.solve_dev takes them, in place allowed"""
        first, second = self._solvers(trans)
        first.solve_dev(b_ptr, ldb, x_ptr, ldx, k, trans, stream)
        second.solve_dev(x_ptr, ldx, x_ptr, ldx, k, trans, stream)

    def solve(self, b, trans="N"):
        """the same for a host array b (1-D, or 2-D in Fortran order), as TriangularSolver.solve takes it"""
        first, second = self._solvers(trans)
        return second.solve(first.solve(b, trans), trans)


def ilu0(mat):
    """the ILU0 object of the host Matrix `mat`, factored on the device"""
    return mat.device_handle().ilu0()


def vector_dot_dev(n, a_ptr, b_ptr, out_ptr, is_complex=False, stream=0):
    """out = <a,b> of n entries in the fixed order of include/sparse_linear_hip.h (conj(a) . b on packed complex
    vectors, is_complex=True); device pointers (ints), out one double or one packed pair; enqueues on `stream`, no sync"""
    check("spl_vector_dot_dev",
          lib().spl_vector_dot_dev(int(n), 2 if is_complex else 1, C.c_void_p(a_ptr), C.c_void_p(b_ptr),
                                   C.c_void_p(out_ptr), C.c_void_p(stream)))


def vector_dots_dev(n, k, V_ptr, ldv, w_ptr, out_ptr, is_complex=False, stream=0):
    """out[i] = <V[:, i], w>, i < k, in ONE pass over w (spl_vector_dots_dev): column i of V starts ldv entries after
    column i - 1, ldv >= n, 1 <= k <= 128; every value is vector_dot_dev's bit for bit.  Device pointers (ints), out k
    doubles or packed pairs; enqueues on `stream`, no sync"""
    check("spl_vector_dots_dev",
          lib().spl_vector_dots_dev(int(n), 2 if is_complex else 1, int(k), C.c_void_p(V_ptr), int(ldv), C.c_void_p(w_ptr),
                                    C.c_void_p(out_ptr), C.c_void_p(stream)))


def vector_gram_dev(n, k, l, V_ptr, ldv, W_ptr, ldw, G_ptr, ldg, upper=False, is_complex=False, stream=0):
    """G[i][j] = <V[:, i], W[:, j]>, i < k, j < l, in ONE pass (spl_vector_gram_dev): V and W are column blocks in
    vector_dots_dev's layout (ldv, ldw >= n), G is column major with ldg >= k; 1 <= k, l <= 128.  ``upper`` writes only
    i <= j and leaves the rest of G alone.  Every entry is vector_dot_dev's bit for bit.  Device pointers (ints);
    enqueues on `stream`, no sync"""
    check("spl_vector_gram_dev",
          lib().spl_vector_gram_dev(int(n), 2 if is_complex else 1, int(k), int(l), C.c_void_p(V_ptr), int(ldv),
                                    C.c_void_p(W_ptr), int(ldw), C.c_void_p(G_ptr), int(ldg), 1 if upper else 0,
                                    C.c_void_p(stream)))


class _PreconditionedSolver(_ffi.Handle):
    """What KrylovSolver and GMRESSolver share: the handle, the preconditioner vocabulary (None, an ``ILU0``, an ``AMG``,
    ``"jacobi"``, ``"sgs"``, ``"amg"`` or a ``(T1, mid, T2)`` triple), ``info`` and the vector plumbing of ``solve``.  A
    subclass names its C calls (``_CALLS``: set_preconditioner, set_preconditioner_amg, info, free) and has
    ``solve_dev`` and ``_solve_host``."""
    REASONS = ("converged", "max_iter", "breakdown", "non_finite")
    DEFAULT_MAXITER = 20000
    _NAME = None
    _CALLS = None

    def _begin(self, A, M):
        _ffi.Handle.__init__(self, self._CALLS["free"])
        self.A = A
        self.parts = (None, None, None)
        self.amg = None   # the AMG in use: M itself, or the one "amg" made here
        self._owned = []  # what "jacobi", "sgs" and "amg" made here
        self._M = M       # an ILU0 stays alive with its solvers

    def free(self):
        _ffi.Handle.free(self)
        for part in self._owned:
            part.free()
        self._owned = []

    def _diagonal(self):
        import torch
        inf = self.A.info()
        with torch.cuda.device(inf["device"]):
            d = torch.empty(max(inf["nrows_global"], 1), dtype=torch.complex128 if self.A.is_complex else torch.float64,
                            device="cuda")
            self.A.take_diag_dev(d.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.current_stream().synchronize()
        return d[:inf["nrows_global"]]

    def set_preconditioner(self, M):
        """replaces the preconditioner (the forms of the class docstring)"""
        owned = []
        set_parts, set_amg = self._CALLS["set_preconditioner"], self._CALLS["set_preconditioner_amg"]
        if isinstance(M, AMG) or (isinstance(M, str) and M == "amg"):
            cycle = M
            if isinstance(M, str):  # built here with the defaults, and freed with the solver
                cycle = AMG(self.A)
                owned = [cycle]
            check(set_amg, getattr(lib(), set_amg)(self.handle, cycle.handle))
            for part in self._owned:
                part.free()
            self._owned, self.parts, self._M, self.amg = owned, (None, None, None), cycle, cycle
            return
        if M is None:
            parts = (None, None, None)
        elif isinstance(M, ILU0):
            parts = (M.lower, None, M.upper)
        elif isinstance(M, str) and M == "jacobi":
            parts = (None, 1.0 / self._diagonal(), None)
        elif isinstance(M, str) and M == "sgs":
            lower, upper = self.A.triangular("lower"), self.A.triangular("upper")
            owned = [lower, upper]
            parts = (lower, self._diagonal(), upper)
        elif isinstance(M, (tuple, list)) and len(M) == 3:
            parts = tuple(M)
        else:
            raise ValueError("%s: M %r; None, an ILU0, an AMG, 'jacobi', 'sgs', 'amg' or a (T1, mid, T2) triple "
                             "is needed" % (self._NAME, M))
        t1, mid, t2 = parts
        if mid is not None:
            n, cplx = self.info()["n"], self.A.is_complex
            import torch
            want = torch.complex128 if cplx else torch.float64
            if not (isinstance(mid, torch.Tensor) and mid.is_cuda and mid.dtype == want and mid.dim() == 1
                    and int(mid.shape[0]) == n and (n <= 1 or mid.stride(0) == 1)):
                _oops(self._NAME, "the middle part must be a contiguous torch device vector of %d %s entries" % (n, want))
        check(set_parts,
              getattr(lib(), set_parts)(self.handle, t1.handle if t1 is not None else None,
                                        C.c_void_p(mid.data_ptr()) if mid is not None else None,
                                        t2.handle if t2 is not None else None))
        for part in self._owned:
            part.free()
        self._owned, self.parts, self._M, self.amg = owned, parts, M, None

    def info(self):
        out = np.zeros(8, dtype=I64)
        check(self._CALLS["info"], getattr(lib(), self._CALLS["info"])(self.handle, _ffi.p_i64(out)))
        d = dict(zip(self.INFO_KEYS, (int(v) for v in out)))
        d.update(complex=bool(d["flags"] & 1), T1=bool(d["flags"] & 2), mid=bool(d["flags"] & 4), T2=bool(d["flags"] & 8),
                 amg=bool(d["flags"] & 16))
        return d

    def _maxiter(self, maxiter):
        if maxiter is None:
            return min(10 * self.info()["n"], self.DEFAULT_MAXITER)
        return int(maxiter)

    def solve(self, b, x0=None, rtol=1e-8, atol=0.0, maxiter=None, check_every=0):
        """(x, result dict) with A x = b.  b (and x0): numpy arrays, or torch tensors on the device (x is one then and
        the solve runs on torch's current stream); float64 on a real object, complex128 on a complex one"""
        where = self._NAME + ".solve"
        inf = self.info()
        n, cplx = inf["n"], inf["complex"]
        a, want, is_tensor = _vector_arg(where, b, (n,), cplx, "right-hand side", "right-hand side")
        if x0 is not None:
            x0 = _vector_arg(where, x0, (n,), cplx, "a start", "start", is_tensor)[0]
        if is_tensor:
            import torch
            with torch.cuda.device(b.device):
                bb = b.contiguous()
                x = torch.empty(max(n, 1), dtype=want, device=b.device)[:n]
                if x0 is not None:
                    x.copy_(x0)
                res = self.solve_dev(bb.data_ptr(), x.data_ptr(), x0 is not None, rtol, atol, maxiter, check_every,
                                     True, torch.cuda.current_stream().cuda_stream)
            return x, res
        a = np.ascontiguousarray(a)
        x = np.zeros(n, dtype=want)
        if x0 is not None:
            x[:] = x0
        maxiter = self._maxiter(maxiter)
        if check_every:  # the host-vector call has no such argument: through device tensors
            import torch
            with torch.cuda.device(self.A.info()["device"]):
                db = torch.from_numpy(a).cuda()
                dx = torch.from_numpy(x).cuda()
                res = self.solve_dev(db.data_ptr(), dx.data_ptr(), x0 is not None, rtol, atol, maxiter, check_every,
                                     True, torch.cuda.current_stream().cuda_stream)
                return dx.cpu().numpy(), res
        return x, self._solve_host(a, x, x0 is not None, rtol, atol, maxiter)


class KrylovSolver(_PreconditionedSolver):
    """Owner of a ``void *K`` from ``spl_krylov_create``: preconditioned CG or BiCGSTAB on a whole square device handle
    (csrc/krylov.hip), real or complex, every scalar of the iteration in device memory.  The iterates, the iteration
    count and the residual history are those of the serial restatement in include/sparse_linear_hip.h bit for bit.

    ``M``: None; an ``ILU0``; ``"jacobi"`` (1 / diag(A)); ``"sgs"`` (symmetric Gauss-Seidel: tril(A), diag(A), triu(A));
    or a triple ``(T1, mid, T2)`` of a TriangularSolver or None, a torch device vector of n entries or None, and a
    TriangularSolver or None, applied as ``z = T2^-1 (mid * (T1^-1 r))``.  The object keeps references to A and to the
    parts of M, so nothing it borrows is collected under it; ``parts`` is the triple in use.  An ``AMG`` object, or
    ``"amg"`` (one built here with the defaults and freed with the solver), makes its V-cycle the preconditioner
    instead of the triple; ``amg`` is the one in use."""
    METHODS = {"cg": _ffi.SPL_KRYLOV_cg, "bicgstab": _ffi.SPL_KRYLOV_bicgstab}
    REASONS = ("converged", "max_iter", "breakdown", "non_finite")
    INFO_KEYS = ("n", "method", "flags", "device_bytes", "solves", "iterations", "launches_per_iteration", "reserved")
    DEFAULT_MAXITER = 20000

    _NAME = "KrylovSolver"
    _CALLS = {"set_preconditioner": "spl_krylov_set_preconditioner",
              "set_preconditioner_amg": "spl_krylov_set_preconditioner_amg", "info": "spl_krylov_info",
              "free": "spl_krylov_free"}

    def __init__(self, A, method="cg", M=None):
        if method not in self.METHODS:
            raise ValueError("KrylovSolver: method %r; 'cg' or 'bicgstab' is needed" % (method,))
        self._begin(A, M)
        self.method = method
        check("spl_krylov_create", lib().spl_krylov_create(A.handle, self.METHODS[method], C.byref(self._h)))
        self.set_preconditioner(M)

    @classmethod
    def _result(cls, result, history):
        it, reason = int(result[0]), int(result[1])
        out = {"iterations": it, "reason": reason, "reason_name": cls.REASONS[reason], "converged": reason == 0,
               "spmvs": int(result[2]), "preconditioner_applications": int(result[3])}
        if history is not None:
            out["history"] = history[:it + 1].copy()
        return out

    def solve_dev(self, b_ptr, x_ptr, use_x0=False, rtol=1e-8, atol=0.0, maxiter=None, check_every=0, history=True,
                  stream=0):
        """device pointers (ints) to b and x (n doubles, or packed pairs); use_x0: x holds the start.  Enqueues on
        `stream` and returns after the solve's last synchronisation with the result dict (iterations, reason, spmvs,
        preconditioner_applications, history)"""
        maxiter = self._maxiter(maxiter)
        result = np.zeros(4, dtype=I64)
        hist = np.zeros(maxiter + 1, dtype=F64) if history else None
        check("spl_krylov_solve_dev",
              lib().spl_krylov_solve_dev(self.handle, C.c_void_p(b_ptr), C.c_void_p(x_ptr), 1 if use_x0 else 0,
                                         float(rtol), float(atol), maxiter, int(check_every), _ffi.p_i64(result),
                                         p_f64(hist) if history else None, C.c_void_p(stream)))
        return self._result(result, hist)

    def _solve_host(self, a, x, use_x0, rtol, atol, maxiter):
        result = np.zeros(4, dtype=I64)
        hist = np.zeros(maxiter + 1, dtype=F64)
        check("spl_krylov_solve",
              lib().spl_krylov_solve(self.handle, p_f64(a.view(F64)), p_f64(x.view(F64)), 1 if use_x0 else 0,
                                     float(rtol), float(atol), maxiter, _ffi.p_i64(result), p_f64(hist)))
        return self._result(result, hist)


class GMRESSolver(_PreconditionedSolver):
    """Owner of a ``void *G`` from ``spl_gmres_create``: right-preconditioned restarted GMRES(restart) on a whole square
    device handle (csrc/gmres.hip), real or complex, for unsymmetric and indefinite systems.  The orthogonalisation is
    classical Gram-Schmidt done twice on the fused multi-vector inner product; every scalar stays in device memory, and
    x, the counts, the history and the residuals are those of the header's sequence bit for bit.  ``M`` as KrylovSolver
    takes it.  The result dict has ``cycles`` and ``residual`` (the true residual norm of the last cycle start)
    and ``estimate`` (the rotations' estimate at the last close) besides KrylovSolver's keys."""
    INFO_KEYS = ("n", "restart", "flags", "device_bytes", "solves", "iterations", "launches", "reserved")
    RESULT_KEYS = ("iterations", "reason", "cycles", "spmvs", "preconditioner_applications", "reserved")
    _NAME = "GMRESSolver"
    _CALLS = {"set_preconditioner": "spl_gmres_set_preconditioner",
              "set_preconditioner_amg": "spl_gmres_set_preconditioner_amg", "info": "spl_gmres_info",
              "free": "spl_gmres_free"}

    def __init__(self, A, restart=30, M=None):
        restart = int(restart)
        if not 1 <= restart <= 128:
            raise ValueError("GMRESSolver: restart %r; 1 ... 128 is needed" % (restart,))
        self._begin(A, M)
        self.restart = restart
        check("spl_gmres_create", lib().spl_gmres_create(A.handle, restart, C.byref(self._h)))
        self.set_preconditioner(M)

    @classmethod
    def _result(cls, result, history, residual):
        out = dict(zip(cls.RESULT_KEYS, (int(v) for v in result)))
        del out["reserved"]
        it, reason = out["iterations"], out["reason"]
        out.update(reason_name=cls.REASONS[reason], converged=reason == 0, residual=float(residual[0]),
                   estimate=float(residual[1]))
        if history is not None:
            out["history"] = history[:it + 1].copy()
        return out

    def solve_dev(self, b_ptr, x_ptr, use_x0=False, rtol=1e-8, atol=0.0, maxiter=None, check_every=0, history=True,
                  stream=0):
        """device pointers (ints) to b and x (n doubles, or packed pairs); use_x0: x holds the start.  Enqueues on
        `stream` and returns after the solve's last synchronisation with the result dict; check_every: cycles between
        two looks at the status block (0: every cycle)"""
        maxiter = self._maxiter(maxiter)
        result, residual = np.zeros(6, dtype=I64), np.zeros(2, dtype=F64)
        hist = np.zeros(maxiter + 1, dtype=F64) if history else None
        check("spl_gmres_solve_dev",
              lib().spl_gmres_solve_dev(self.handle, C.c_void_p(b_ptr), C.c_void_p(x_ptr), 1 if use_x0 else 0,
                                        float(rtol), float(atol), maxiter, int(check_every), _ffi.p_i64(result),
                                        p_f64(hist) if history else None, p_f64(residual), C.c_void_p(stream)))
        return self._result(result, hist, residual)

    def _solve_host(self, a, x, use_x0, rtol, atol, maxiter):
        result, residual = np.zeros(6, dtype=I64), np.zeros(2, dtype=F64)
        hist = np.zeros(maxiter + 1, dtype=F64)
        check("spl_gmres_solve",
              lib().spl_gmres_solve(self.handle, p_f64(a.view(F64)), p_f64(x.view(F64)), 1 if use_x0 else 0,
                                    float(rtol), float(atol), maxiter, _ffi.p_i64(result), p_f64(hist), p_f64(residual)))
        return self._result(result, hist, residual)


def gmres(mat, b, M=None, x0=None, restart=30, rtol=1e-8, atol=0.0, maxiter=None):
    """(x, result dict) with mat x = b by right-preconditioned restarted GMRES on the device; mat: a host Matrix; M as
    KrylovSolver takes it.  The dict is bicgstab's plus ``cycles``, ``residual`` (the true residual norm) and
    ``estimate``"""
    G = mat.device_handle().gmres(restart, M)
    try:
        return G.solve(b, x0, rtol, atol, maxiter)
    finally:
        G.free()


def vector_rotate_dev(n, m, k, V_ptr, ldv, Y_ptr, ldy, out_ptr=None, ldo=0, is_complex=False, stream=0,
                      Y_is_complex=False):
    """V[:, :k] <- V Y in place (out_ptr None), or out = V Y (spl_vector_rotate_dev): V has m columns of n entries, ldv
    entries apart; Y is a REAL m x k device matrix, column major, ldy >= m; 1 <= k <= m <= 128.  Column i is
    Y[0][i] v_0 + Y[1][i] v_1 + ... summed in ascending order.  ``Y_is_complex``: Y holds packed pairs and V is complex
    (spl_vector_rotate_z_dev).  Device pointers (ints); enqueues on `stream`, no sync"""
    if Y_is_complex:
        if not is_complex:
            raise ValueError("vector_rotate_dev: a complex Y needs complex vectors (is_complex=True)")
        check("spl_vector_rotate_z_dev",
              lib().spl_vector_rotate_z_dev(int(n), 2, int(m), int(k), C.c_void_p(V_ptr), int(ldv), C.c_void_p(Y_ptr),
                                            int(ldy), C.c_void_p(out_ptr) if out_ptr else None, int(ldo),
                                            C.c_void_p(stream)))
        return
    check("spl_vector_rotate_dev",
          lib().spl_vector_rotate_dev(int(n), 2 if is_complex else 1, int(m), int(k), C.c_void_p(V_ptr), int(ldv),
                                      C.c_void_p(Y_ptr), int(ldy), C.c_void_p(out_ptr) if out_ptr else None, int(ldo),
                                      C.c_void_p(stream)))


class _EigenPairs(object):
    """What EigenSolver and LOBPCGSolver share: the host buffers of a solve, the result dict, and the end of ``solve``
    that makes room for the vectors and cuts them to the pairs found.  A subclass has ``RESULT_KEYS``, ``REASONS`` and
    ``_history_entries(out, history)``, the entries of the history its solve wrote."""

    @classmethod
    def _buffers(cls, nev, rounds, history=True):
        """values, residuals, result and the history of a solve of at most `rounds` restarts or iterations"""
        return (np.zeros(max(nev, 1), dtype=F64), np.zeros(max(nev, 1), dtype=F64),
                np.zeros(len(cls.RESULT_KEYS), dtype=I64), np.zeros(max(rounds, 0) + 1, dtype=F64) if history else None)

    @classmethod
    def _result(cls, result, values, residuals, history):
        out = dict(zip(cls.RESULT_KEYS, (int(v) for v in result)))
        pairs = out["pairs"]
        out.update(reason_name=cls.REASONS[out["reason"]], converged=out["reason"] == 0,
                   residuals=residuals[:pairs].copy())
        if history is not None:
            out["history"] = history[:cls._history_entries(out, history)].copy()
        return values[:pairs].copy(), out

    @staticmethod
    def _solve_pairs(nev, n, start, want, is_tensor, on_device, on_host):
        """(values, vectors, result dict) from the start, one column after the other: a device tensor, solved by
        ``on_device(start_ptr, vectors_ptr, stream)`` on torch's current stream, or a numpy array, solved by
        ``on_host(start, vectors)``; both return (values, result dict)"""
        if is_tensor:
            import torch
            with torch.cuda.device(start.device):
                start = start.contiguous()
                X = torch.zeros((max(nev, 1), max(n, 1)), dtype=want, device=start.device)
                values, res = on_device(start.data_ptr(), X.data_ptr(), torch.cuda.current_stream().cuda_stream)
            return values, X[:res["pairs"], :n].T, res
        start = np.ascontiguousarray(start)
        X = np.zeros((max(nev, 1), max(n, 1)), dtype=want)
        values, res = on_host(p_f64(start.view(F64)), p_f64(X.view(F64)))
        return values, X[:res["pairs"], :n].T.copy(), res


class EigenSolver(_ffi.Handle, _EigenPairs):
    """Owner of a ``void *E`` from ``spl_eigsh_create``: thick-restart Lanczos with full reorthogonalisation on a whole
    square Hermitian device handle (csrc/eigsh.hip), real or complex, with a basis of ``ncv`` columns.  Directly on A it
    finds the ends of the spectrum; with ``sigma`` it works on ``(A - sigma I)^-1``, applied by a CG ``KrylovSolver``
    built here on ``A.lin(1, I, -sigma)`` with the preconditioner ``M`` (as KrylovSolver takes it), and ``which="LM"``
    then finds the eigenvalues nearest sigma.  ``which`` orders the OPERATOR's values.  Values, vectors, residuals,
    history and counts are those of the sequence in include/sparse_linear_hip.h bit for bit.  A single-vector Lanczos
    finds one copy of a multiple eigenvalue."""
    WHICH = {"LA": _ffi.SPL_EIGSH_largest_algebraic, "SA": _ffi.SPL_EIGSH_smallest_algebraic,
             "LM": _ffi.SPL_EIGSH_largest_magnitude}
    REASONS = ("converged", "max_restarts", "invariant_subspace", "non_finite", "inner_solve_failed")
    INFO_KEYS = ("n", "ncv", "flags", "device_bytes", "solves", "cycles", "launches", "reserved")
    RESULT_KEYS = ("reason", "cycles", "applications", "pairs", "inner_iterations", "jacobi_sweeps")
    DEFAULT_INNER_MAXITER = 20000

    def __init__(self, A, ncv=20, sigma=None, M=None, inner_rtol=1e-12, inner_atol=0.0, inner_maxiter=None):
        ncv = int(ncv)
        if not 2 <= ncv <= 128:
            raise ValueError("EigenSolver: ncv %r; 2 ... 128 is needed" % (ncv,))
        _ffi.Handle.__init__(self, "spl_eigsh_free")
        self.A, self.ncv, self.sigma = A, ncv, None
        self.shifted = self.inner = None
        check("spl_eigsh_create", lib().spl_eigsh_create(A.handle, ncv, C.byref(self._h)))
        if sigma is not None:
            self.set_inverse(sigma, M, inner_rtol, inner_atol, inner_maxiter)

    def free(self):
        _ffi.Handle.free(self)
        self._drop_inner()

    def _drop_inner(self):
        if self.inner is not None:
            self.inner.free()
        self.shifted = self.inner = None

    def set_inverse(self, sigma, M=None, inner_rtol=1e-12, inner_atol=0.0, inner_maxiter=None):
        """the operator becomes (A - sigma I)^-1 by CG on ``A.lin(1, I, -sigma)`` with the preconditioner M; sigma None:
        back to A itself"""
        if sigma is None:
            check("spl_eigsh_set_inverse", lib().spl_eigsh_set_inverse(self.handle, None, 0.0, 0.0, 0.0, 0))
            self._drop_inner()
            self.sigma = None
            return
        n = self.info()["n"]
        shifted = self.A.lin(1.0, DeviceMatrix.ident(n, complex=self.A.is_complex), -float(sigma))
        inner = KrylovSolver(shifted, "cg", M)
        if inner_maxiter is None:
            inner_maxiter = min(10 * n, self.DEFAULT_INNER_MAXITER)
        try:
            check("spl_eigsh_set_inverse",
                  lib().spl_eigsh_set_inverse(self.handle, inner.handle, float(sigma), float(inner_rtol),
                                              float(inner_atol), int(inner_maxiter)))
        except Exception:
            inner.free()
            raise
        self._drop_inner()
        self.shifted, self.inner, self.sigma = shifted, inner, float(sigma)

    def info(self):
        out = np.zeros(8, dtype=I64)
        check("spl_eigsh_info", lib().spl_eigsh_info(self.handle, _ffi.p_i64(out)))
        d = dict(zip(self.INFO_KEYS, (int(v) for v in out)))
        d.update(complex=bool(d["flags"] & 1), inverse=bool(d["flags"] & 2))
        return d

    @classmethod
    def _which(cls, which):
        if which not in cls.WHICH:
            raise ValueError("EigenSolver: which %r; 'LA', 'SA' or 'LM' is needed" % (which,))
        return cls.WHICH[which]

    @staticmethod
    def _history_entries(out, history):
        return out["cycles"] + 1

    def solve_dev(self, nev, v0_ptr, vectors_ptr, ldx, which="LA", tol=1e-10, atol=0.0, max_restarts=1000, history=True,
                  stream=0):
        """device pointers (ints) to v0 (n entries) and the vectors (nev columns, ldx entries apart).  Enqueues on
        `stream` and returns (values, result dict) after the solve's last synchronisation; the dict has reason, cycles,
        applications, pairs, inner_iterations, jacobi_sweeps, residuals and history"""
        nev, max_restarts = int(nev), int(max_restarts)
        values, residuals, result, hist = self._buffers(nev, max_restarts, history)
        check("spl_eigsh_solve_dev",
              lib().spl_eigsh_solve_dev(self.handle, nev, self._which(which), float(tol), float(atol), max_restarts,
                                        C.c_void_p(v0_ptr), p_f64(values), C.c_void_p(vectors_ptr), int(ldx),
                                        p_f64(residuals), _ffi.p_i64(result), p_f64(hist) if history else None,
                                        C.c_void_p(stream)))
        return self._result(result, values, residuals, hist)

    def default_start(self):
        """numpy.random.default_rng(0).standard_normal of n entries (complex: both parts)"""
        inf = self.info()
        rng = np.random.default_rng(0)
        if inf["complex"]:
            return (rng.standard_normal(inf["n"]) + 1j * rng.standard_normal(inf["n"])).astype(C128)
        return rng.standard_normal(inf["n"])

    def solve(self, nev, which="LA", tol=1e-10, atol=0.0, max_restarts=1000, v0=None):
        """(values, vectors, result dict): vectors has one column per pair returned.  v0: None (default_start), a numpy
        array, or a torch tensor on the device (the vectors are one then and the solve runs on torch's current
        stream); float64 on a real object, complex128 on a complex one"""
        where = "EigenSolver.solve"
        inf = self.info()
        n, cplx = inf["n"], inf["complex"]
        nev, max_restarts = int(nev), int(max_restarts)
        start, want, is_tensor = _vector_arg(where, self.default_start() if v0 is None else v0, (n,), cplx, "a start",
                                             "start")

        def on_host(start_p, vectors_p):
            values, residuals, result, hist = self._buffers(nev, max_restarts)
            check("spl_eigsh_solve",
                  lib().spl_eigsh_solve(self.handle, nev, self._which(which), float(tol), float(atol), max_restarts, start_p,
                                        p_f64(values), vectors_p, max(n, 1), p_f64(residuals), _ffi.p_i64(result),
                                        p_f64(hist)))
            return self._result(result, values, residuals, hist)

        return self._solve_pairs(nev, n, start, want, is_tensor,
                                 lambda v0_ptr, vectors_ptr, stream: self.solve_dev(
                                     nev, v0_ptr, vectors_ptr, max(n, 1), which, tol, atol, max_restarts, True, stream),
                                 on_host)


def default_ncv(n, nev):
    """min(n, max(2 nev + 1, 20)), capped at 128"""
    return min(int(n), max(2 * int(nev) + 1, 20), 128)


def eigsh(mat, nev, which="LA", ncv=None, sigma=None, M=None, tol=1e-10, atol=0.0, max_restarts=1000, v0=None,
          inner_rtol=1e-12, inner_atol=0.0, inner_maxiter=None):
    """(values, vectors, result dict): nev eigenpairs of the Hermitian host Matrix `mat` by thick-restart Lanczos on the
    device (DeviceMatrix.eigsh)"""
    return mat.device_handle().eigsh(nev, which, ncv, sigma, M, tol, atol, max_restarts, v0, inner_rtol, inner_atol,
                                     inner_maxiter)


class LOBPCGSolver(_PreconditionedSolver, _EigenPairs):
    """Owner of a ``void *L`` from ``spl_lobpcg_create``: LOBPCG on a whole square Hermitian device handle
    (csrc/lobpcg.hip), real or complex, with a block of ``block`` columns (1 ... 42) and the preconditioner ``M`` (as
    KrylovSolver takes it) applied inside the iteration, one application per column and iteration.  A block method: it
    returns every copy of a multiple eigenvalue its block has room for.  Values, vectors, residuals, history and counts
    are those of the sequence in include/sparse_linear_hip.h bit for bit.  Converged columns are not locked."""
    REASONS = ("converged", "max_iter", "start_rank_deficient", "non_finite")
    INFO_KEYS = ("n", "block", "flags", "device_bytes", "solves", "iterations", "launches", "reserved")
    RESULT_KEYS = ("reason", "iterations", "spmv_columns", "pairs", "preconditioner_applications", "jacobi_sweeps",
                   "columns_dropped", "synchronisations")
    _NAME = "LOBPCGSolver"
    _CALLS = {"set_preconditioner": "spl_lobpcg_set_preconditioner",
              "set_preconditioner_amg": "spl_lobpcg_set_preconditioner_amg", "info": "spl_lobpcg_info",
              "free": "spl_lobpcg_free"}

    def __init__(self, A, block, M=None, B=None):
        block = int(block)
        if not 1 <= block <= 42:
            raise ValueError("LOBPCGSolver: block %r; 1 ... 42 is needed" % (block,))
        self._begin(A, M)
        self.block = block
        self.B = None
        check("spl_lobpcg_create", lib().spl_lobpcg_create(A.handle, block, C.byref(self._h)))
        self.set_preconditioner(M)
        if B is not None:
            self.set_mass(B)

    def set_mass(self, B):
        """the generalized problem A x = lambda B x with the Hermitian positive definite DeviceMatrix B (a mass matrix),
        which this object keeps alive; None: the standard problem again, and the memory of B S is released.  The vectors
        of a solve are B-orthonormal and the residuals are those of the pencil"""
        if B is not None and not isinstance(B, DeviceMatrix):
            raise ValueError("LOBPCGSolver.set_mass: B %r; a DeviceMatrix or None is needed" % (B,))
        check("spl_lobpcg_set_mass", lib().spl_lobpcg_set_mass(self.handle, B.handle if B is not None else None))
        self.B = B

    def info(self):
        d = _PreconditionedSolver.info(self)
        d.update(generalized=bool(d["flags"] & 32), mass_columns=d["reserved"])
        return d

    @staticmethod
    def _history_entries(out, history):
        return min(out["iterations"], len(history) - 1) + 1

    @staticmethod
    def _which(largest):
        return _ffi.SPL_EIGSH_largest_algebraic if largest else _ffi.SPL_EIGSH_smallest_algebraic

    def solve_dev(self, nev, X0_ptr, ldx0, vectors_ptr, ldx, largest=False, tol=1e-8, atol=0.0, maxiter=200, history=True,
                  stream=0):
        """device pointers (ints) to X0 (block columns, ldx0 entries apart; not changed) and the vectors (nev columns,
        ldx entries apart).  Enqueues on `stream` and returns (values, result dict) after the solve's last
        synchronisation"""
        nev, maxiter = int(nev), int(maxiter)
        values, residuals, result, hist = self._buffers(nev, maxiter, history)
        check("spl_lobpcg_solve_dev",
              lib().spl_lobpcg_solve_dev(self.handle, nev, self._which(largest), float(tol), float(atol), maxiter,
                                         C.c_void_p(X0_ptr), int(ldx0), p_f64(values), C.c_void_p(vectors_ptr), int(ldx),
                                         p_f64(residuals), _ffi.p_i64(result), p_f64(hist) if history else None,
                                         C.c_void_p(stream)))
        return self._result(result, values, residuals, hist)

    def solve(self, X0, nev=None, largest=False, tol=1e-8, atol=0.0, maxiter=200):
        """(values, vectors, result dict): X0 is the start block, n x block, a numpy array or a torch tensor on the device
        (the vectors are one then and the solve runs on torch's current stream); float64 on a real object, complex128
        on a complex one.  nev: the pairs wanted, default the whole block"""
        where = "LOBPCGSolver.solve"
        inf = self.info()
        n, cplx, block = inf["n"], inf["complex"], inf["block"]
        nev, maxiter = block if nev is None else int(nev), int(maxiter)
        start, want, is_tensor = _vector_arg(where, X0, (n, block), cplx, "a start", "start")

        def on_host(start_p, vectors_p):
            values, residuals, result, hist = self._buffers(nev, maxiter)
            check("spl_lobpcg_solve",
                  lib().spl_lobpcg_solve(self.handle, nev, self._which(largest), float(tol), float(atol), maxiter, start_p,
                                         max(n, 1), p_f64(values), vectors_p, max(n, 1), p_f64(residuals),
                                         _ffi.p_i64(result), p_f64(hist)))
            return self._result(result, values, residuals, hist)

        return self._solve_pairs(nev, n, start.T, want, is_tensor,  # .T: one column after the other
                                 lambda X0_ptr, vectors_ptr, stream: self.solve_dev(
                                     nev, X0_ptr, max(n, 1), vectors_ptr, max(n, 1), largest, tol, atol, maxiter, True, stream),
                                 on_host)


def lobpcg(mat, X0, nev=None, largest=False, M=None, tol=1e-8, atol=0.0, maxiter=200, B=None):
    """(values, vectors, result dict): the nev smallest (or largest) eigenpairs of the Hermitian host Matrix `mat` by
    LOBPCG on the device from the start block X0 (DeviceMatrix.lobpcg); B: a Hermitian positive definite host Matrix
    for mat x = lambda B x"""
    return mat.device_handle().lobpcg(X0, nev, largest, M, tol, atol, maxiter,
                                      B.device_handle() if B is not None else None)


def vector_update_pair_dev(n, k, V_ptr, ldv, BV_ptr, ldbv, coef_ptr, w_ptr, bw_ptr, q_ptr=None, is_complex=False, stream=0):
    """w = ((w - c_0 v_0) - c_1 v_1) - ... and bw = ((bw - c_0 (Bv)_0) - ...) over the k columns of V and BV with the same
    k coefficients, in ONE launch (spl_vector_update_pair_dev): the columns are laid out as vector_dots_dev's (ldv, ldbv
    >= n), 1 <= k <= 128.  With q_ptr, one double receives Re<w, bw> of the results, the real part of vector_dot_dev's
    value bit for bit.  Device pointers (ints); enqueues on `stream`, no sync"""
    check("spl_vector_update_pair_dev",
          lib().spl_vector_update_pair_dev(int(n), 2 if is_complex else 1, int(k), C.c_void_p(V_ptr), int(ldv),
                                           C.c_void_p(BV_ptr), int(ldbv), C.c_void_p(coef_ptr), C.c_void_p(w_ptr),
                                           C.c_void_p(bw_ptr), C.c_void_p(q_ptr) if q_ptr else None, C.c_void_p(stream)))


def _krylov(method, mat, b, M, x0, rtol, atol, maxiter):
    K = mat.device_handle().krylov(method, M)
    try:
        return K.solve(b, x0, rtol, atol, maxiter)
    finally:
        K.free()


def cg(mat, b, M=None, x0=None, rtol=1e-8, atol=0.0, maxiter=None):
    """(x, result dict) with mat x = b by preconditioned CG on the device; mat: a host Matrix, Hermitian positive
    definite; M as KrylovSolver takes it"""
    return _krylov("cg", mat, b, M, x0, rtol, atol, maxiter)


def bicgstab(mat, b, M=None, x0=None, rtol=1e-8, atol=0.0, maxiter=None):
    """(x, result dict) with mat x = b by right-preconditioned BiCGSTAB on the device; mat: a host Matrix"""
    return _krylov("bicgstab", mat, b, M, x0, rtol, atol, maxiter)


class _DeviceArray(object):
    """n entries of device memory the library lends, in the form torch.as_tensor reads without a copy"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class AMG(_ffi.Handle):
    """Owner of a ``void *M`` from ``spl_amg_create``: the aggregation AMG hierarchy of a whole square device handle and
    its V-cycle (csrc/amg.hip), real or complex.  Every level is the composition of the public handle operations that
    include/sparse_linear_hip.h lists, and ``apply`` is that header's cycle bit for bit.  ``KrylovSolver(A, method, M=amg)``
    takes it as the preconditioner; one AMG may serve several solvers.  The object keeps a reference to A, which it
    borrows as level 0."""
    OPTIONS = ("seed", "sweeps", "coarse_size", "max_levels", "coarse_sweeps", "plain")
    INFO_KEYS = ("n", "levels", "nnz_total", "nnz_fine", "coarsest_n", "tail_first", "device_bytes", "flags")
    AGGREGATE_KEYS = ("n", "aggregates", "rounds", "largest", "smallest", "max_degree", "launches", "phase2")

    def __init__(self, A, **options):
        unknown = sorted(set(options) - set(self.OPTIONS))
        if unknown:
            raise TypeError("AMG: unknown option %s; the options are %s" % (", ".join(unknown), ", ".join(self.OPTIONS)))
        _ffi.Handle.__init__(self, "spl_amg_free")
        self.A = A
        opt = np.zeros(8, dtype=I64)
        opt[0] = int(options.get("seed", 0))
        opt[1] = int(options.get("sweeps", 0))
        opt[2] = int(options.get("coarse_size", 0))
        opt[3] = int(options.get("max_levels", 0))
        opt[4] = int(options.get("coarse_sweeps", 0))
        opt[5] = 1 if options.get("plain", False) else 0
        check("spl_amg_create", lib().spl_amg_create(A.handle, _ffi.p_i64(opt), C.byref(self._h)))

    def info(self):
        out = np.zeros(8, dtype=I64)
        check("spl_amg_info", lib().spl_amg_info(self.handle, _ffi.p_i64(out)))
        d = dict(zip(self.INFO_KEYS, (int(v) for v in out)))
        d.update(zero_diagonal=bool(d["flags"] & 1), complex=bool(d["flags"] & 2),
                 operator_complexity=d["nnz_total"] / float(d["nnz_fine"]) if d["nnz_fine"] else 1.0)
        return d

    @property
    def levels(self):
        return self.info()["levels"]

    def level(self, l):
        """level l as a dict: ``A``, ``P``, ``R`` (borrowed DeviceMatrix views that do not free; P and R None on the
        coarsest level), ``w`` (a copy of the weights as a torch device tensor) and ``dims`` = (n_l, n_{l+1} or 0)"""
        import torch
        ha, hp, hr, pw = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        dims = np.zeros(2, dtype=I64)
        check("spl_amg_level",
              lib().spl_amg_level(self.handle, int(l), C.byref(ha), C.byref(hp), C.byref(hr), C.byref(pw), _ffi.p_i64(dims)))
        inf = self.info()
        n = int(dims[0])
        with torch.cuda.device(self.A.info()["device"]):
            if n:
                lent = _DeviceArray(pw.value, n, "<c16" if inf["complex"] else "<f8")
                w = torch.as_tensor(lent, device="cuda").clone()  # the object's memory is read, the copy is the caller's
            else:
                w = torch.empty(0, dtype=torch.complex128 if inf["complex"] else torch.float64, device="cuda")
        view = lambda h: DeviceMatrix._borrowed(h.value, self) if h.value else None  # noqa: E731
        return {"A": view(ha), "P": view(hp), "R": view(hr), "w": w, "dims": (n, int(dims[1]))}

    def apply_dev(self, b_ptr, x_ptr, stream=0):
        """x = cycle(0, b): device pointers (ints) to n doubles, or packed pairs; b and x different arrays; enqueues on
        `stream`, no sync"""
        check("spl_amg_apply_dev",
              lib().spl_amg_apply_dev(self.handle, C.c_void_p(b_ptr), C.c_void_p(x_ptr), C.c_void_p(stream)))

    def apply(self, b):
        """the cycle of b: a numpy array for a numpy array, a device tensor (on torch's current stream) for one"""
        inf = self.info()
        n, cplx = inf["n"], inf["complex"]
        a, want, is_tensor = _vector_arg("AMG.apply", b, (n,), cplx, "a vector")
        if is_tensor:
            import torch
            with torch.cuda.device(b.device):
                bb = b.contiguous()
                x = torch.empty(max(n, 1), dtype=want, device=b.device)[:n]
                self.apply_dev(bb.data_ptr(), x.data_ptr(), torch.cuda.current_stream().cuda_stream)
            return x
        a = np.ascontiguousarray(a)
        x = np.zeros(n, dtype=want)
        check("spl_amg_apply", lib().spl_amg_apply(self.handle, p_f64(a.view(F64)), p_f64(x.view(F64))))
        return x


def amg(mat, **options):
    """the AMG object of the host Matrix `mat`, built on the device"""
    return mat.device_handle().amg(**options)


def vector_permute_dev(n, perm_ptr, in_ptr, out_ptr, inverse=False, is_complex=False, stream=0):
    """out[k] = in[perm[k]], or with inverse out[perm[k]] = in[k], for n entries moved as bits (spl_vector_permute_dev);
    device pointers (ints), perm int32, in and out different arrays; enqueues on `stream`, no sync"""
    check("spl_vector_permute_dev",
          lib().spl_vector_permute_dev(int(n), 2 if is_complex else 1, C.c_void_p(perm_ptr), 1 if inverse else 0,
                                       C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.c_void_p(stream)))


class Coloring(object):
    """The multicolour ordering of a whole square device handle (csrc/coloring.hip, spl_matrix_color): ``colors`` and
    ``perm`` are torch int32 device tensors of n entries, ``offsets`` a numpy array of ncolors + 1 class boundaries in
    ``perm``.  colors is the serial first-fit colouring in the priority order of the seed's hash, exactly; perm lists
    the vertices by colour and then by ascending index.  ``permute(A)`` is P A P^T, whose triangular solves and ILU(0)
    have at most ``ncolors`` levels; ``krylov`` solves with it and answers in the original numbering."""
    INFO_KEYS = ("n", "colors", "rounds", "largest_class", "smallest_class", "max_degree", "launches", "reserved")

    def __init__(self, A, seed=0):
        handle = A.handle  # a freed handle is refused here
        _ffi.require_gpu()
        import torch
        inf = A.info()
        n = inf["nrows_global"]
        self.A, self.seed, self.n = A, int(seed), n
        dev = torch.device("cuda", inf["device"])
        out = np.zeros(8, dtype=I64)
        off = _ffi.c_i64_p()
        with torch.cuda.device(dev):
            colors = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            perm = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            torch.cuda.current_stream().synchronize()  # the call runs on the default stream
            check("spl_matrix_color",
                  lib().spl_matrix_color(handle, _ffi.SPL_COLOR_hash, self.seed, C.c_void_p(colors.data_ptr()),
                                         C.c_void_p(perm.data_ptr()), C.byref(off), _ffi.p_i64(out)))
        self._info = tuple(int(v) for v in out)
        self.ncolors = self._info[1]
        self.colors, self.perm = colors[:n], perm[:n]
        self.offsets = _ffi.take_malloced(off, self.ncolors + 1, C.c_int64, I64)

    def info(self):
        return dict(zip(self.INFO_KEYS, self._info))

    def permute(self, A=None):
        """P A P^T as a new handle: A.select(perm, perm); A: the coloured handle, or another of its size"""
        return (self.A if A is None else A).select(self.perm, self.perm)

    def _move(self, v, inverse, what):
        import torch
        is_tensor = isinstance(v, torch.Tensor)
        t = v if is_tensor else torch.from_numpy(np.ascontiguousarray(v)).to(self.perm.device)
        if not (t.is_cuda and t.dtype in (torch.float64, torch.complex128) and tuple(t.shape) == (self.n,)):
            _oops(what, "a float64 or complex128 vector of %d entries, numpy or on the device, is needed" % self.n)
        with torch.cuda.device(t.device):
            t = t.contiguous()
            out = torch.empty(max(self.n, 1), dtype=t.dtype, device=t.device)[:self.n]
            vector_permute_dev(self.n, self.perm.data_ptr(), t.data_ptr(), out.data_ptr(), inverse,
                               t.dtype == torch.complex128, torch.cuda.current_stream().cuda_stream)
            return out if is_tensor else out.cpu().numpy()

    def to_permuted(self, v):
        """v in the new numbering, out[k] = v[perm[k]]: a numpy array for a numpy array, a device tensor for one"""
        return self._move(v, False, "Coloring.to_permuted")

    def from_permuted(self, v):
        """back to the original numbering, out[perm[k]] = v[k]"""
        return self._move(v, True, "Coloring.from_permuted")

    def krylov(self, method="cg", M=None):
        """a MulticolorKrylov: CG or BiCGSTAB on P A P^T with the preconditioner built there from None, 'jacobi',
        'sgs', 'ilu0' or a (T1, mid, T2) triple in the new numbering"""
        return MulticolorKrylov(self, method, M)


class MulticolorKrylov(object):
    """KrylovSolver on B = P A P^T of a Coloring.  ``solve`` permutes b (and x0), runs the ordinary solver on B and
    returns x in the original numbering with the usual result dict.  ``B``, ``solver`` and, for M = 'ilu0', ``ilu``
    (the ILU0 of B made here) are open to the caller; free() releases all three.  The solver borrows ilu's two
    triangular solvers: after ``ilu.refactor(...)``, which replaces them, call ``solver.set_preconditioner(ilu)``."""

    def __init__(self, coloring, method="cg", M=None):
        if method not in KrylovSolver.METHODS:
            raise ValueError("Coloring.krylov: method %r; 'cg' or 'bicgstab' is needed" % (method,))
        self.coloring = coloring
        self.B = coloring.permute()
        self.ilu = None
        if isinstance(M, str) and M == "ilu0":
            self.ilu = M = ILU0(self.B)
        self.solver = KrylovSolver(self.B, method, M)

    def solve(self, b, x0=None, rtol=1e-8, atol=0.0, maxiter=None, check_every=0):
        c = self.coloring
        x, res = self.solver.solve(c.to_permuted(b), None if x0 is None else c.to_permuted(x0), rtol, atol, maxiter,
                                   check_every)
        return c.from_permuted(x), res

    def info(self):
        return self.solver.info()

    def free(self):
        self.solver.free()
        if self.ilu is not None:
            self.ilu.free()
        self.B.free()


def multicolor(mat, seed=0):
    """the Coloring of the host Matrix `mat`, computed on the device"""
    return mat.device_handle().coloring(seed)


# ---- accessors ------------------------------------------------------------------------------

def nonZero(mat):
    return int(mat.pointers[-1])  # Sparse.hs:115-117


def cmap(f, mat):
    return Matrix(mat.ncols, mat.nrows, mat.pointers, mat.indices, f(mat.values))  # :119-121


def scale(x, mat):
    return cmap(lambda v: v * x, mat)  # :123-125


def slice(mat, c):  # noqa: A001 - the reference's name
    """(indices, values) of column c as a sparse vector of length nrows (Sparse.hs:175-182)."""
    if c >= mat.ncols:
        _oops("slice", "column out of range")
    s, e = int(mat.pointers[c]), int(mat.pointers[c + 1])
    return mat.nrows, mat.indices[s:e], mat.values[s:e]


def toColumns(mat):
    return [slice(mat, c) for c in range(mat.ncols)]  # :381-383


# ---- construction on the device ---------------------------------------------------------------

def compress(nrows, ncols, rows, cols, vals):
    """COO -> CSC, duplicates summed, explicit zeros kept (Sparse.hs:184-255)."""
    rows = np.asarray(rows)
    cols = np.asarray(cols)
    vals = np.asarray(vals)
    if np.iscomplexobj(vals) and len(rows) == len(cols) == len(vals):
        # complex addition is componentwise: the duplicate sums of the two real runs ARE the complex sums
        re = compress(nrows, ncols, rows, cols, vals.real)
        im = compress(nrows, ncols, rows, cols, vals.imag)
        return Matrix(ncols, nrows, re.pointers, re.indices, re.values + 1j * im.values)
    vals = np.asarray(vals, dtype=F64)
    if len(rows) != len(cols):
        _oops("compress", "row and column array lengths differ")
    if len(rows) != len(vals):
        _oops("compress", "row and value array lengths differ")
    _ffi.require_gpu()
    r32, c32 = _checked_i32(rows, nrows, "row"), _checked_i32(cols, ncols, "column")
    ap = np.zeros(ncols + 1, dtype=np.int32)
    ai, ax, bad = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
    st = lib().spl_compress(nrows, ncols, len(r32), p_i32(r32), p_i32(c32), p_f64(as_f64(vals)), p_i32(ap),
                            C.byref(ai), C.byref(ax), C.byref(bad))
    if st == SPL_ERROR_index_out_of_bounds:
        k = bad.value
        if not (0 <= rows[k] < nrows):
            _oops("compress", "row index out of bounds (0,%d) at %d" % (nrows, k))
        _oops("compress", "column index out of bounds (0,%d) at %d" % (ncols, k))
    check("spl_compress", st)
    nz = int(ap[ncols])
    return Matrix(ncols, nrows, ap.astype(I64), _ffi.take_malloced(ai, nz, C.c_int, I64),
                  _ffi.take_malloced(ax, nz, C.c_double, F64))


def _checked_i32(a, bound, what):
    """int64 -> int32 narrowing that keeps out-of-range values out of range"""
    a = np.asarray(a, dtype=I64)
    lim = np.iinfo(np.int32)
    return np.ascontiguousarray(np.where((a < lim.min) | (a > lim.max), -1, a), dtype=np.int32)


def fromTriples(nr, nc, triples):
    triples = list(triples)
    rows = [t[0] for t in triples]
    cols = [t[1] for t in triples]
    vals = [t[2] for t in triples]
    return compress(nr, nc, rows, cols, vals)  # Sparse.hs:357-363


def transpose(mat):
    """Counting-sort transpose (Sparse.hs:301-329); also the CSC -> CSR converter."""
    if mat.is_complex:
        re, im = (transpose(m) for m in mat._parts())
        return Matrix(re.ncols, re.nrows, re.pointers, re.indices, re.values + 1j * im.values)
    _ffi.require_gpu()
    nr, nc, ap, ai, ax = mat._tuple32()
    nz = int(ap[nc])
    tp = np.zeros(nr + 1, dtype=np.int32)
    ti = np.zeros(max(nz, 1), dtype=np.int32)
    tx = np.zeros(max(nz, 1), dtype=F64)
    check("spl_transpose", lib().spl_transpose(nr, nc, p_i32(ap), p_i32(ai), p_f64(ax), p_i32(tp), p_i32(ti),
                                              p_f64(tx)))
    return Matrix(nr, nc, tp.astype(I64), ti[:nz].astype(I64), tx[:nz])


def ctrans(mat):
    """omap conj . transpose (Sparse.hs:371-375); conj is the identity on Double"""
    t = transpose(mat)
    return cmap(np.conj, t) if t.is_complex else t


def hermitian(mat):
    return ctrans(mat) == mat  # :377-379


# ---- SpMV ---------------------------------------------------------------------------------------

def axpy_(mat, xs, ys):
    """in place ys <- A xs + ys (Sparse.hs:433-453); ys is a float64 numpy array."""
    if len(xs) != mat.ncols:
        _oops("axpy_", "column dimension %d does not match operand dimension %d" % (mat.ncols, len(xs)))
    if len(ys) != mat.nrows:
        _oops("axpy_", "row dimension %d does not match result dimension %d" % (mat.nrows, len(ys)))
    want = C128 if mat.is_complex else F64
    if not (isinstance(ys, np.ndarray) and ys.dtype == want and ys.flags.c_contiguous):
        raise TypeError("axpy_: ys must be a contiguous %s array (it is updated in place)" % np.dtype(want).name)
    mat.device_handle().gaxpy(xs, ys)  # Complex Double: the native kernel of csrc/spmv_z.hip


def axpy(mat, x, y):
    dt = C128 if mat.is_complex else F64
    y = np.array(y, dtype=dt)  # U.thaw _y (Sparse.hs:459)
    axpy_(mat, np.asarray(x, dtype=dt), y)
    return y


def mulV(mat, x):
    if mat.is_complex or np.iscomplexobj(x):
        # Complex Double (Sparse.hs:465-466): native packed-complex kernel (csrc/spmv_z.hip); a real matrix
        # applied to a complex vector is promoted as the reference's types would demand
        x = np.ascontiguousarray(x, dtype=C128)
        if len(x) != mat.ncols:
            _oops("axpy_", "column dimension %d does not match operand dimension %d" % (mat.ncols, len(x)))
        m = mat if mat.is_complex else cmap(lambda v: v.astype(C128), mat)
        return m.device_handle().mulv(x)
    x = np.asarray(x, dtype=F64)
    if len(x) != mat.ncols:
        _oops("axpy_", "column dimension %d does not match operand dimension %d" % (mat.ncols, len(x)))
    return mat.device_handle().mulv(x)  # Sparse.hs:464-471


def mulVT(mat, x):
    """A^T x — a gather on the CSC arrays themselves."""
    _ffi.require_gpu()
    x = as_f64(x)
    nr, nc, ap, ai, ax = mat._tuple32()
    y = np.zeros(nc, dtype=F64)
    st = lib().spl_gaxpy_t(nr, nc, p_i32(ap), p_i32(ai), p_f64(ax), len(x), p_f64(x), nc, p_f64(y))
    if st == SPL_ERROR_dimension_mismatch:
        _oops("axpy_", "row dimension %d does not match operand dimension %d" % (nr, len(x)))
    check("spl_gaxpy_t", st)
    return y


def mulM(matA, matB):
    """sparse x dense (Sparse.hs:473-498); matB is a 2-D array (rows x cols)."""
    if matA.is_complex or np.iscomplexobj(matB):
        # Complex Double (the SPECIALIZE instance of Sparse.hs:475): the real operand is promoted as mulV promotes it
        B = np.ascontiguousarray(matB, dtype=C128)
        if matA.ncols != B.shape[0]:
            _oops("mulM", "inner dimension mismatch")
        _ffi.require_gpu()
        m = matA if matA.is_complex else cmap(lambda v: v.astype(C128), matA)
        nr, nc, ap, ai, az = m._tuple32()
        out = np.zeros((nr, B.shape[1]), dtype=C128)
        check("spl_mulm_z", lib().spl_mulm_z(nr, nc, p_i32(ap), p_i32(ai), p_f64(az), B.shape[0], B.shape[1],
                                            p_f64(B.view(F64)), p_f64(out.view(F64))))
        return out
    B = np.ascontiguousarray(matB, dtype=F64)
    if matA.ncols != B.shape[0]:
        _oops("mulM", "inner dimension mismatch")
    _ffi.require_gpu()
    nr, nc, ap, ai, ax = matA._tuple32()
    out = np.zeros((nr, B.shape[1]), dtype=F64)
    check("spl_mulm", lib().spl_mulm(nr, nc, p_i32(ap), p_i32(ai), p_f64(ax), B.shape[0], B.shape[1],
                                    p_f64(B), p_f64(out)))
    return out


# ---- SpGEMM / sparse add ---------------------------------------------------------------------------

def _take_matrix(where, st, nr, nc, cp, ci, cx):
    check(where, st)
    ncols = nc.value
    ptrs = _ffi.take_malloced(cp, ncols + 1, C.c_int, I64)
    nz = int(ptrs[ncols])
    return Matrix(ncols, nr.value, ptrs, _ffi.take_malloced(ci, nz, C.c_int, I64),
                  _ffi.take_malloced(cx, nz, C.c_double, F64))


def mm(matA, matB):
    """C = A B (Sparse.hs:691-702): union pattern, cancellation keeps a stored 0."""
    if matA.ncols != matB.nrows:
        _oops("mm", "inner dimension mismatch")
    if matA.is_complex or matB.is_complex:
        # Complex Double: pattern from the real kernels, values accumulated in the reference's order with
        # Data.Complex's arithmetic (csrc/spgemm_z.hip, spl_spgemm_z)
        _ffi.require_gpu()
        a = (matA if matA.is_complex else cmap(lambda v: v.astype(C128), matA))._tuple32()
        b = (matB if matB.is_complex else cmap(lambda v: v.astype(C128), matB))._tuple32()
        nr, nc = C.c_int(), C.c_int()
        cp, ci, cz = C.c_void_p(), C.c_void_p(), C.c_void_p()
        st = lib().spl_spgemm_z(a[0], a[1], p_i32(a[2]), p_i32(a[3]), p_f64(a[4]), b[0], b[1], p_i32(b[2]),
                                p_i32(b[3]), p_f64(b[4]), C.byref(nr), C.byref(nc), C.byref(cp), C.byref(ci),
                                C.byref(cz))
        check("spl_spgemm_z", st)
        ncols = nc.value
        ptrs = _ffi.take_malloced(cp, ncols + 1, C.c_int, I64)
        nz = int(ptrs[ncols])
        return Matrix(ncols, nr.value, ptrs, _ffi.take_malloced(ci, nz, C.c_int, I64),
                      _ffi.take_malloced(cz, 2 * nz, C.c_double, F64).view(C128))
    _ffi.require_gpu()
    a, b = matA._tuple32(), matB._tuple32()
    nr, nc = C.c_int(), C.c_int()
    cp, ci, cx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = lib().spl_spgemm(a[0], a[1], p_i32(a[2]), p_i32(a[3]), p_f64(a[4]), b[0], b[1], p_i32(b[2]),
                          p_i32(b[3]), p_f64(b[4]), C.byref(nr), C.byref(nc), C.byref(cp), C.byref(ci),
                          C.byref(cx))
    return _take_matrix("spl_spgemm", st, nr, nc, cp, ci, cx)


def lin(alpha, matA, beta, matB):
    """alpha A + beta B (Sparse.hs:426-431 over glin :401-424)."""
    if matA.nrows != matB.nrows:
        _oops("glin", "row number mismatch")
    if matA.ncols != matB.ncols:
        _oops("glin", "column number mismatch")
    if matA.is_complex or matB.is_complex or np.iscomplexobj(alpha) or np.iscomplexobj(beta):
        # Complex Double (what Feast.hs:216 calls: `lin (-1) matA _ze matB`): the native packed-complex kernel,
        # Data.Complex's evaluation order (spl_lin_z)
        _ffi.require_gpu()
        a = (matA if matA.is_complex else cmap(lambda v: v.astype(C128), matA))._tuple32()
        b = (matB if matB.is_complex else cmap(lambda v: v.astype(C128), matB))._tuple32()
        al = np.array([complex(alpha).real, complex(alpha).imag], dtype=F64)
        be = np.array([complex(beta).real, complex(beta).imag], dtype=F64)
        nr, nc = C.c_int(), C.c_int()
        cp, ci, cz = C.c_void_p(), C.c_void_p(), C.c_void_p()
        st = lib().spl_lin_z(p_f64(al), a[0], a[1], p_i32(a[2]), p_i32(a[3]), p_f64(a[4].view(F64)),
                             p_f64(be), b[0], b[1], p_i32(b[2]), p_i32(b[3]), p_f64(b[4].view(F64)),
                             C.byref(nr), C.byref(nc), C.byref(cp), C.byref(ci), C.byref(cz))
        check("spl_lin_z", st)
        ncols = nc.value
        ptrs = _ffi.take_malloced(cp, ncols + 1, C.c_int, I64)
        nz = int(ptrs[ncols])
        return Matrix(ncols, nr.value, ptrs, _ffi.take_malloced(ci, nz, C.c_int, I64),
                      _ffi.take_malloced(cz, 2 * nz, C.c_double, F64).view(C128))
    _ffi.require_gpu()
    a, b = matA._tuple32(), matB._tuple32()
    nr, nc = C.c_int(), C.c_int()
    cp, ci, cx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = lib().spl_lin(float(alpha), a[0], a[1], p_i32(a[2]), p_i32(a[3]), p_f64(a[4]), float(beta), b[0],
                       b[1], p_i32(b[2]), p_i32(b[3]), p_f64(b[4]), C.byref(nr), C.byref(nc), C.byref(cp),
                       C.byref(ci), C.byref(cx))
    return _take_matrix("spl_lin", st, nr, nc, cp, ci, cx)


# ---- structural combinators: concatenations are host-side index plumbing (pure data movement
# between host arrays); kronecker and takeDiag run on the device ----------------------------------

def _lengths(mat):
    return np.diff(mat.pointers)


def diag(values):
    values = np.asarray(values)
    values = values.astype(C128) if np.iscomplexobj(values) else values.astype(F64)
    n = len(values)
    return Matrix(n, n, np.arange(n + 1, dtype=I64), np.arange(n, dtype=I64), values)  # :650-657


def ident(n):
    return diag(np.ones(n, dtype=F64))  # :667-669


def zeros(nrows, ncols):
    return Matrix(ncols, nrows, np.zeros(ncols + 1, dtype=I64), np.zeros(0, dtype=I64),
                  np.zeros(0, dtype=F64))  # :671-677


def takeDiag(mat):
    """diagonal as a dense vector, 0 where nothing is stored (Sparse.hs:636-648); on the device"""
    if mat.is_complex:
        re, im = mat._parts()
        return takeDiag(re) + 1j * takeDiag(im)
    _ffi.require_gpu()
    a = mat._tuple32()
    out = np.zeros(min(mat.nrows, mat.ncols), dtype=F64)
    check("spl_take_diag", lib().spl_take_diag(a[0], a[1], p_i32(a[2]), p_i32(a[3]), p_f64(a[4]), p_f64(out)))
    return out


def _assemble(blocks, row_off, col_off, nrows, ncols):
    """place CSC blocks at (row_off, col_off) of an nrows x ncols result on the device (spl_assemble_blocks, the
    kernels of csrc/assemble_handles.hip): the one call behind hcat / vcat / fromBlocks / fromBlocksDiag"""
    _ffi.require_gpu()
    k = len(blocks)
    cplx = any(m.is_complex for m in blocks)
    keep = []  # the int32 / float64 copies must outlive the call
    nr, nc = (C.c_int * k)(), (C.c_int * k)()
    ro, co = (C.c_int * k)(*[int(v) for v in row_off]), (C.c_int * k)(*[int(v) for v in col_off])
    ap, ai, ax = (C.c_void_p * k)(), (C.c_void_p * k)(), (C.c_void_p * k)()
    for b, m in enumerate(blocks):
        vals = m.values.astype(C128) if cplx else m.values
        t = (as_i32(m.pointers), as_i32(m.indices), as_f64(vals.view(F64) if cplx else vals))
        keep.append(t)
        nr[b], nc[b] = m.nrows, m.ncols
        ap[b], ai[b], ax[b] = t[0].ctypes.data, t[1].ctypes.data, t[2].ctypes.data
    cp, ci, cx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    fn = lib().spl_assemble_blocks
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                   C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    st = fn(k, nr, nc, ap, ai, ax, 2 if cplx else 1, ro, co, int(nrows), int(ncols), C.byref(cp), C.byref(ci), C.byref(cx))
    check("spl_assemble_blocks", st)
    ptrs = _ffi.take_malloced(cp, ncols + 1, C.c_int, np.int32)
    nz = int(ptrs[-1])
    idx = _ffi.take_malloced(ci, max(nz, 1), C.c_int, np.int32)[:nz]
    val = _ffi.take_malloced(cx, max(nz, 1) * (2 if cplx else 1), C.c_double, F64)[:nz * (2 if cplx else 1)]
    return Matrix(ncols, nrows, ptrs, idx, val.view(C128) if cplx else val)


def hcat(mats):
    """hcat (Sparse.hs:504-522), assembled on the device"""
    mats = list(mats)
    if not mats:
        _oops("hcat", "empty list")
    if any(m.nrows != mats[0].nrows for m in mats):
        _oops("hcat", "nrows mismatch")
    widths = [m.ncols for m in mats]
    return _assemble(mats, [0] * len(mats), np.concatenate([[0], np.cumsum(widths)])[:-1], mats[0].nrows, sum(widths))


def hjoin(a, b):
    return hcat([a, b])


def vcat(mats):
    """vcat (Sparse.hs:528-559), assembled on the device: blocks stacked in list order inside every column"""
    mats = list(mats)
    if not mats:
        _oops("vcat", "empty list")
    ncols = mats[0].ncols
    if any(m.ncols != ncols for m in mats):
        _oops("vcat", "ncols mismatch")
    heights = [m.nrows for m in mats]
    return _assemble(mats, np.concatenate([[0], np.cumsum(heights)])[:-1], [0] * len(mats), sum(heights), ncols)


def vjoin(a, b):
    return vcat([a, b])


def _block_grid(blocks, height, width):
    """adjustDims of fromBlocks (Sparse.hs:563-587) for a grid with None = zero block: (placed blocks listed row-major,
    their row offsets, their column offsets, nrows, ncols); height / width read a block's dimensions"""
    rows = [list(r) for r in blocks]
    ncb = max(len(r) for r in rows)
    cols = [[r[c] for r in rows if c < len(r)] for c in range(ncb)]

    def spec(groups, dim, what):
        out = []
        for g in groups:
            ds = [dim(m) for m in g if m is not None]
            if not ds:
                _oops("fromBlocks", "underspecified " + what)
            if any(d != ds[0] for d in ds):
                _oops("fromBlocks", "incompatible " + what)
            out.append(ds[0])
        return out

    heights = spec(rows, height, "heights")
    widths = spec(cols, width, "widths")
    roff = np.concatenate([[0], np.cumsum(heights)])
    # hcat of a block row fails in the reference when the rows' widths differ in total (vcat: ncols mismatch)
    totals = [sum(widths[:len(r)]) for r in rows]
    if any(t != totals[0] for t in totals):
        _oops("vcat", "ncols mismatch")
    coff = np.concatenate([[0], np.cumsum(widths)])
    placed, ro, co = [], [], []
    for r, row in enumerate(rows):
        for c, m in enumerate(row):
            if m is not None:
                placed.append(m)
                ro.append(int(roff[r]))
                co.append(int(coff[c]))
    return placed, ro, co, int(roff[-1]), int(totals[0])


def _diag_grid(blocks):
    """fromBlocksDiag's rearrangement (Sparse.hs:589-597): blocks given by (super-)diagonals -> a grid for fromBlocks"""
    blocks = [list(b) for b in blocks]
    n = len(blocks)
    trans = [[b[i] for b in blocks if i < len(b)] for i in range(max(len(b) for b in blocks))]
    out = []
    for k, as_ in enumerate(trans):
        as_ = as_ + [None] * (n - len(as_))
        cut = len(as_) - k
        out.append(as_[cut:] + as_[:cut])
    return out


def fromBlocks(blocks):
    """[[Maybe Matrix]] -> Matrix, None = zero block (Sparse.hs:563-587): vcat . map hcat . adjustDims in one
    device assembly — block (r, c) sits at (sum of the heights above, sum of the widths to the left); the call
    stacks blocks that share columns by ascending row offset whatever order they are listed in."""
    placed, ro, co, nrows, ncols = _block_grid(blocks, lambda m: m.nrows, lambda m: m.ncols)
    if not placed:  # every block a zero block cannot happen: heights would be underspecified
        return zeros(nrows, ncols)
    return _assemble(placed, ro, co, nrows, ncols)


def fromBlocksDiag(blocks):
    """blocks given by (super-)diagonals (Sparse.hs:589-597)."""
    return fromBlocks(_diag_grid(blocks))


def blockDiag(mats):
    mats = list(mats)
    n = len(mats)
    return fromBlocksDiag([list(mats)] + [[None] * n for _ in range(n - 1)])  # :659-665


def kronecker(matA, matB):
    """Kronecker product (Sparse.hs:597-634), assembled on the device: column ja*ncols(B)+jb holds
    the rows ia*nrows(B)+ib with values b*a."""
    if matA.is_complex or matB.is_complex:
        ar, ai = (matA if matA.is_complex else cmap(lambda v: v.astype(C128), matA))._parts()
        br, bi = (matB if matB.is_complex else cmap(lambda v: v.astype(C128), matB))._parts()
        rr, ii, ri, ir = kronecker(ar, br), kronecker(ai, bi), kronecker(ar, bi), kronecker(ai, br)
        # all four share the pattern of the complex product; (ar + i ai)(br + i bi) componentwise
        return Matrix(rr.ncols, rr.nrows, rr.pointers, rr.indices,
                      (rr.values - ii.values) + 1j * (ri.values + ir.values))
    _ffi.require_gpu()
    a, b = matA._tuple32(), matB._tuple32()
    nr, nc = C.c_int(), C.c_int()
    cp, ci, cx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = lib().spl_kronecker(a[0], a[1], p_i32(a[2]), p_i32(a[3]), p_f64(a[4]), b[0], b[1], p_i32(b[2]),
                             p_i32(b[3]), p_f64(b[4]), C.byref(nr), C.byref(nc), C.byref(cp), C.byref(ci),
                             C.byref(cx))
    return _take_matrix("spl_kronecker", st, nr, nc, cp, ci, cx)


def subMatrix(origin, shape, mat):
    """subMatrix (r0, c0) (nr, nc) mat: the nr x nc window of `mat` whose top left corner is (r0, c0), indices relative
    to the window — the operation the signature and the two guards of Sparse.hs:704-729 document.  The reference's body
    is untested and does not compute it: (1) `U.slice ix0 nix` passes an END where a LENGTH belongs, (2) the kept row
    indices are not shifted by r0, (3) `computePtrs nc _indices` builds the column pointers from ROW indices.  Those
    bits are not reproduced; the documented operation is what is computed, on the device: one upload, the handle call
    (spl_matrix_submatrix), one export."""
    r0, c0 = (int(v) for v in origin)
    nr, nc = (int(v) for v in shape)
    if min(r0, c0, nr, nc) < 0:
        _oops("subMatrix", "negative origin or size")
    if r0 + nr > mat.nrows:
        _oops("subMatrix", "range exceeds input row size")
    if c0 + nc > mat.ncols:
        _oops("subMatrix", "range exceeds input column size")
    _ffi.require_gpu()
    if mat.is_complex:
        # the CSC fields of a complex handle are export_csr of its transpose (include/sparse_linear_hip.h)
        cp, ri, v = DeviceMatrix.from_csc_complex(mat).submatrix(r0, c0, nr, nc).transpose().export_csr()
    else:
        cp, ri, v = DeviceMatrix.from_csc(mat).submatrix(r0, c0, nr, nc).export_csc()
    return Matrix(nc, nr, cp, ri, v.copy())


def pack(mat):
    """dense copy (Sparse.hs:679-689)"""
    out = np.zeros((mat.nrows, mat.ncols), dtype=mat.values.dtype)
    cols = np.repeat(np.arange(mat.ncols), _lengths(mat))
    out[mat.indices, cols] = mat.values
    return out


def outer(sliceC, sliceR):
    """outer product of a sparse column and a sparse row vector (Sparse.hs:331-355);
    both given as (length, indices, values).  Mirrors the reference's naming,
    in which `sliceC` supplies the column dimension."""
    ncols, indicesC, valuesC = sliceC
    nrows, indicesR, valuesR = sliceR
    lenR = len(valuesR)
    lens = np.zeros(ncols + 1, dtype=I64)
    lens[np.asarray(indicesC, dtype=I64)] = lenR
    ptrs = np.concatenate([[0], np.cumsum(lens)]).astype(I64)
    idx = np.tile(np.asarray(indicesR, dtype=I64), len(valuesC))
    val = (np.asarray(valuesC, dtype=F64)[:, None] * np.asarray(valuesR, dtype=F64)[None, :]).ravel()
    return Matrix(ncols, nrows, ptrs[:ncols + 1], idx, val)
